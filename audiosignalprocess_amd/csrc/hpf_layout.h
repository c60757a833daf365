// hpf_layout.h -- what the high-pass filter's and the level estimator's kernels, host code and CPU build agree on:
// the state structs' sizes and the LDS tile both kernels stage their frames through.
//
// The tile: a workgroup is one wave, a lane owns one row (a stream-channel's frame for the filter, up to
// kTileSamples samples of a stream's frame for the meter).  The rows of a workgroup are consecutive in global
// memory, so the tile is filled and emptied with consecutive lanes on consecutive dwords (or, where a row is not a
// whole number of aligned dwords, and for float audio, consecutive samples).  In LDS a row is kTilePitch = 81 dwords
// apart from the next: lane l reads its sample pair j at dword 81 l + j, and 81 is odd, so the 32 lanes of a
// ds_read_b32 group fall in 32 distinct banks.
#ifndef ASP_HPF_LAYOUT_H_
#define ASP_HPF_LAYOUT_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_hpf.h"
#include "asp_level.h"

#if defined(__HIPCC__)
#define HPF_HD __host__ __device__
#else
#define HPF_HD
#endif

namespace asphpf {

static_assert(sizeof(AspHpfState) == 16, "AspHpfState is 16 bytes: one dwordx4 per stream-channel");
static_assert(sizeof(AspLevelState) == 8, "AspLevelState is two dwords");

constexpr int kWave = 64;                        // rows of a tile: lanes of the one wave of a workgroup
constexpr int kTileSamples = ASP_HPF_MAX_SAMPLES;
constexpr int kTileWords = kTileSamples / 2;
constexpr int kTilePitch = kTileWords + 1;       // odd
constexpr int kTileBatch = 16;                   // global loads a lane has in flight while the tile is filled
static_assert(kTilePitch % 2 == 1, "an even pitch puts lanes l and l + 16 on one bank");
static_assert(ASP_LEVEL_MAX_SAMPLES % kTileSamples == 0, "the meter walks a channel's row in whole tiles");

// FloatS16ToS16 (common_audio/include/audio_util.h)
HPF_HD inline int16_t float_s16_to_s16(float v) {
  const float kMaxRound = 32767 - 0.5f, kMinRound = -32768 + 0.5f;
  if (v > 0) return v >= kMaxRound ? (int16_t)32767 : (int16_t)(v + 0.5f);
  return v <= kMinRound ? (int16_t)-32768 : (int16_t)(v - 0.5f);
}

#if defined(__HIPCC__)   // the kernels' side
__device__ inline void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One element of the tile as global memory has it: G = uint32_t is a sample pair, int16_t a sample, float a FloatS16
// sample.  `col` counts G's within the row.
__device__ inline void tile_put(uint32_t* tile, int row, int col, uint32_t v) { tile[row * kTilePitch + col] = v; }
__device__ inline void tile_put(uint32_t* tile, int row, int col, int16_t v) {
  ((int16_t*)tile)[row * (2 * kTilePitch) + col] = v;
}
__device__ inline void tile_put(uint32_t* tile, int row, int col, float v) {
  ((int16_t*)tile)[row * (2 * kTilePitch) + col] = float_s16_to_s16(v);
}
__device__ inline void tile_get(const uint32_t* tile, int row, int col, uint32_t& v) { v = tile[row * kTilePitch + col]; }
__device__ inline void tile_get(const uint32_t* tile, int row, int col, int16_t& v) {
  v = ((const int16_t*)tile)[row * (2 * kTilePitch) + col];
}
__device__ inline void tile_get(const uint32_t* tile, int row, int col, float& v) {
  v = (float)((const int16_t*)tile)[row * (2 * kTilePitch) + col];
}

// The wave's walk over rows x m elements, 64 consecutive elements a step: lane's element after k steps, as tile
// coordinates and as an element offset into global memory, whose rows are `pitch` elements apart.
struct TileWalk {
  int row, col, q, r, m;
  uint32_t goff, gstep, gwrap;
  __device__ TileWalk(int lane, int m_, uint32_t pitch)
      : row(lane / m_), col(lane % m_), q(kWave / m_), r(kWave % m_), m(m_) {
    goff = (uint32_t)row * pitch + (uint32_t)col;
    gstep = (uint32_t)q * pitch + (uint32_t)r;
    gwrap = pitch - (uint32_t)m_;
  }
  __device__ void step() {
    row += q;
    col += r;
    goff += gstep;
    if (col >= m) {
      col -= m;
      ++row;
      goff += gwrap;
    }
  }
};

// Fills rows [0, rows) x [0, m) of the tile from src.  The wave covers kTileBatch x 64 elements at a time: the loads
// of a batch are issued before the first of them is used, and only the last, partial batch tests its lanes' bounds
// (with a test on every load the staging was bound by its own instructions, not by the loads' latency).
template <typename G>
__device__ inline void tile_load(uint32_t* tile, const G* src, uint32_t pitch, int m, int rows, int lane) {
  const int total = rows * m;   // wave-uniform, as is `done`
  TileWalk w(lane, m, pitch);
  int done = 0;
  for (; done + kTileBatch * kWave <= total; done += kTileBatch * kWave) {
    G v[kTileBatch];
    int ro[kTileBatch], co[kTileBatch];
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k) {
      ro[k] = w.row;
      co[k] = w.col;
      v[k] = src[w.goff];
      w.step();
    }
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k) tile_put(tile, ro[k], co[k], v[k]);
  }
  if (done < total) {
    G v[kTileBatch];
    int ro[kTileBatch], co[kTileBatch];
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k) {
      ro[k] = w.row;
      co[k] = w.col;
      v[k] = w.row < rows ? src[w.goff] : G(0);
      w.step();
    }
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k)
      if (ro[k] < rows) tile_put(tile, ro[k], co[k], v[k]);
  }
}

template <typename G>
__device__ inline void tile_store(const uint32_t* tile, G* dst, uint32_t pitch, int m, int rows, int lane) {
  const int total = rows * m;
  TileWalk w(lane, m, pitch);
  int done = 0;
  for (; done + kTileBatch * kWave <= total; done += kTileBatch * kWave) {
    G v[kTileBatch];
    uint32_t go[kTileBatch];
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k) {
      go[k] = w.goff;
      tile_get(tile, w.row, w.col, v[k]);
      w.step();
    }
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k) dst[go[k]] = v[k];
  }
  if (done < total) {
    G v[kTileBatch] = {};
    uint32_t go[kTileBatch];
    int ro[kTileBatch];
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k) {
      go[k] = w.goff;
      ro[k] = w.row;
      if (w.row < rows) tile_get(tile, w.row, w.col, v[k]);
      w.step();
    }
#pragma unroll
    for (int k = 0; k < kTileBatch; ++k)
      if (ro[k] < rows) dst[go[k]] = v[k];
  }
}
#endif  // __HIPCC__

}  // namespace asphpf

#endif  // ASP_HPF_LAYOUT_H_
