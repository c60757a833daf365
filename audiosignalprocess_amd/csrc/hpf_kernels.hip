// hpf_kernels.hip -- the batched high-pass filter on gfx950 (include/asp_hpf.h).
//
// The biquad is strictly serial per stream-channel and a frame moves 4 bytes per sample, so the kernel is bound by
// the dependent chain of hpf_core.h's filter_sample, not by memory.  One lane serves a stream-channel, 64 of them
// make a wave, a workgroup is one wave.  A lane keeps its six state words and five
// coefficients in registers across the F frames of a call: the state is loaded once and stored once.  The 64 rows
// of a workgroup's frame are one contiguous piece of the [F][S][C][n] array; it is staged through hpf_layout.h's
// tile, dword accesses with consecutive lanes on consecutive dwords where n is even and the arrays are dword
// aligned (kWords), sample accesses otherwise and for float audio.  Streams of a wave may differ in coefficient
// set; that is a register value, not a branch.  Integer arithmetic: bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "hpf_core.h"

namespace asphpf {

struct HpfArgs {
  AspHpfState* state;   // [U]
  int U, F, n;          // U = S * C stream-channels
  const void* in;       // [F][U][n]
  void* out;
};

namespace {

// T: int16_t or float (FloatS16) audio; kWords: int16 audio moved as dwords
template <typename T, bool kWords>
__global__ void __launch_bounds__(kWave) hpf_frames_kernel(HpfArgs a) {
  __shared__ uint32_t tile[kWave * kTilePitch];
  const int lane = threadIdx.x;
  const int u0 = blockIdx.x * kWave;
  const int rows = a.U - u0 < kWave ? a.U - u0 : kWave;
  const bool active = lane < rows;
  const int n = a.n;
  AspHpfState st;
  if (active) {
    const uint4 w = *(const uint4*)(a.state + u0 + lane);
    __builtin_memcpy(&st, &w, sizeof st);
  } else {
    init_state(st, 0);
  }
  HpfRegs r = load_regs(st);
  const HpfCoeffs c = coeffs(st.coeff_set);
  uint32_t* row = tile + lane * kTilePitch;
  for (int f = 0; f < a.F; ++f) {
    const size_t base = ((size_t)f * a.U + u0) * n;
    if (kWords)
      tile_load(tile, (const uint32_t*)a.in + base / 2, (uint32_t)(n / 2), n / 2, rows, lane);
    else
      tile_load(tile, (const T*)a.in + base, (uint32_t)n, n, rows, lane);
    wsync();
    if (active) {
#pragma unroll 4
      for (int j = 0; j < n / 2; ++j) {
        const uint32_t w = row[j];
        const int32_t o0 = filter_sample(r, c, (int16_t)(w & 0xffff));
        const int32_t o1 = filter_sample(r, c, (int16_t)(w >> 16));
        row[j] = ((uint32_t)o0 & 0xffff) | ((uint32_t)o1 << 16);
      }
      if (n & 1) {
        const uint32_t w = row[n / 2];
        const int32_t o0 = filter_sample(r, c, (int16_t)(w & 0xffff));
        row[n / 2] = ((uint32_t)o0 & 0xffff) | (w & 0xffff0000u);
      }
    }
    wsync();
    if (kWords)
      tile_store(tile, (uint32_t*)a.out + base / 2, (uint32_t)(n / 2), n / 2, rows, lane);
    else
      tile_store(tile, (T*)a.out + base, (uint32_t)n, n, rows, lane);
    wsync();   // the next frame's staging overwrites the tile
  }
  if (active) {
    store_regs(st, r);
    uint4 w;
    __builtin_memcpy(&w, &st, sizeof st);
    *(uint4*)(a.state + u0 + lane) = w;
  }
}

}  // namespace

// is_float: FloatS16 audio.  The dword form needs whole, aligned dwords per row.
hipError_t launch_hpf(const HpfArgs& a, bool is_float, hipStream_t stream) {
  const dim3 grid((a.U + kWave - 1) / kWave), block(kWave);
  const bool words = !is_float && a.n % 2 == 0 && ((uintptr_t)a.in | (uintptr_t)a.out) % 4 == 0;
  if (is_float)
    hipLaunchKernelGGL((hpf_frames_kernel<float, false>), grid, block, 0, stream, a);
  else if (words)
    hipLaunchKernelGGL((hpf_frames_kernel<int16_t, true>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((hpf_frames_kernel<int16_t, false>), grid, block, 0, stream, a);
  return hipGetLastError();
}

}  // namespace asphpf
