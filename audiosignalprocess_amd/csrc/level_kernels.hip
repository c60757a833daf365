// level_kernels.hip -- the batched level estimator on gfx950 (include/asp_level.h).
//
// RMSLevel::Process is one float add per sample in sample order, channel after channel: a dependent chain per
// stream that reads 2 bytes a sample.  One lane serves a stream and walks its C * n samples of a frame in order,
// 64 streams make a wave, a workgroup is one wave.  The sum and the count stay in registers
// across the F frames of a call.  The 64 streams' frame rows are contiguous in the [F][S][C][n] array; they pass
// through hpf_layout.h's tile kTileSamples samples of each row at a time, as dwords where the rows are whole
// aligned dwords (kWords).  The squares and their conversions hang off the add chain; the adds are never
// reassociated.  Float adds of exactly converted integers, round to nearest: bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "level_core.h"

namespace asphpf {

struct LevelArgs {
  AspLevelState* state;   // [S]
  int S, F, row;          // row = C * n samples of a stream's frame
  const int16_t* in;      // [F][S][row]
};

namespace {

template <bool kWords>
__global__ void __launch_bounds__(kWave) level_frames_kernel(LevelArgs a) {
  __shared__ uint32_t tile[kWave * kTilePitch];
  const int lane = threadIdx.x;
  const int s0 = blockIdx.x * kWave;
  const int rows = a.S - s0 < kWave ? a.S - s0 : kWave;
  const bool active = lane < rows;
  AspLevelState st = {0.f, 0};
  if (active) st = a.state[s0 + lane];
  float sum = st.sum_square;
  const uint32_t* row = tile + lane * kTilePitch;
  for (int f = 0; f < a.F; ++f) {
    const size_t base = ((size_t)f * a.S + s0) * a.row;
    for (int c0 = 0; c0 < a.row; c0 += kTileSamples) {
      const int m = a.row - c0 < kTileSamples ? a.row - c0 : kTileSamples;
      if (kWords)
        tile_load(tile, (const uint32_t*)a.in + (base + c0) / 2, (uint32_t)(a.row / 2), m / 2, rows, lane);
      else
        tile_load(tile, a.in + base + c0, (uint32_t)a.row, m, rows, lane);
      wsync();
      if (active) {
#pragma unroll 8
        for (int j = 0; j < m / 2; ++j) {
          const uint32_t w = row[j];
          level_add(sum, (int16_t)(w & 0xffff));
          level_add(sum, (int16_t)(w >> 16));
        }
        if (m & 1) level_add(sum, (int16_t)(row[m / 2] & 0xffff));
      }
      wsync();   // the next piece overwrites the tile
    }
  }
  if (active) {
    st.sum_square = sum;
    level_count(st, (int32_t)((uint32_t)a.F * (uint32_t)a.row));
    a.state[s0 + lane] = st;
  }
}

__global__ void __launch_bounds__(kWave) level_muted_kernel(AspLevelState* state, int count, int32_t length) {
  const int s = blockIdx.x * kWave + threadIdx.x;
  if (s < count) level_count(state[s], length);
}

}  // namespace

hipError_t launch_level(const LevelArgs& a, hipStream_t stream) {
  const dim3 grid((a.S + kWave - 1) / kWave), block(kWave);
  if (a.row % 2 == 0 && (uintptr_t)a.in % 4 == 0)
    hipLaunchKernelGGL(level_frames_kernel<true>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(level_frames_kernel<false>, grid, block, 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_level_muted(AspLevelState* state, int count, int32_t length, hipStream_t stream) {
  hipLaunchKernelGGL(level_muted_kernel, dim3((count + kWave - 1) / kWave), dim3(kWave), 0, stream, state, count, length);
  return hipGetLastError();
}

}  // namespace asphpf
