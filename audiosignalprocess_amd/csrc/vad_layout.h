// vad_layout.h -- the VAD's launch geometry, LDS layout and the C integer semantics the reference relies on
// (int32 wrap, (int16_t) casts, arithmetic right shifts, truncating division), shared by vad_kernels.hip
// and vad_api.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "asp_vad.h"

static_assert(sizeof(AspVadState) == 736, "AspVadState must keep VadInstT's layout");

namespace aspvad {

constexpr int kLanes = 64;         // one wave per workgroup, one stream per lane
constexpr int kInStride = 482;     // staged 10 ms piece, [lane][kInStride] int16: 241 dwords, odd -> no bank conflict
constexpr int kMax8k = 240;        // 30 ms at 8 kHz
constexpr int kInitCheck = 42;

// ---- C integer semantics (all 32-bit arithmetic wraps, as the reference's int32 does on its targets)
__device__ __forceinline__ int wadd(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
__device__ __forceinline__ int wsub(int a, int b) { return (int)((unsigned)a - (unsigned)b); }
__device__ __forceinline__ int wmul(int a, int b) { return (int)((unsigned)a * (unsigned)b); }
__device__ __forceinline__ int wshl(int a, int n) { return (int)((unsigned)a << n); }
__device__ __forceinline__ int s16(int a) { return (int)(int16_t)a; }           // (int16_t) cast
__device__ __forceinline__ int div_w32w16(int num, int den) {                   // WebRtcSpl_DivW32W16
  den = s16(den);
  return den != 0 ? num / den : 0x7FFFFFFF;
}
__device__ __forceinline__ int norm_w32(int a) {                               // WebRtcSpl_NormW32
  return a == 0 ? 0 : __clz(a < 0 ? ~a : a) - 1;
}
__device__ __forceinline__ int norm_u32(unsigned a) { return a == 0 ? 0 : __clz((int)a); }  // NormU32
__device__ __forceinline__ int size_in_bits(unsigned n) { return 32 - __clz((int)n); }      // GetSizeInBits

// ---- mode tables (vad_core.c set_mode_core): over_hang_max_1, over_hang_max_2, individual, total x 3
constexpr int16_t kModeTab[4][4][3] = {
    {{8, 4, 3}, {14, 7, 5}, {24, 21, 24}, {57, 48, 57}},
    {{8, 4, 3}, {14, 7, 5}, {37, 32, 37}, {100, 80, 100}},
    {{6, 3, 2}, {9, 5, 3}, {82, 78, 82}, {285, 260, 285}},
    {{6, 3, 2}, {9, 5, 3}, {94, 94, 94}, {1100, 1050, 1100}}};

__device__ __forceinline__ void mode_table(int mode, int16_t* m1, int16_t* m2, int16_t* ind, int16_t* tot) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    m1[i] = kModeTab[mode][0][i];
    m2[i] = kModeTab[mode][1][i];
    ind[i] = kModeTab[mode][2][i];
    tot[i] = kModeTab[mode][3][i];
  }
}

}  // namespace aspvad
