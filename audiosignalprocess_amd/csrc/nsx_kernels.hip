// nsx_kernels.hip -- the batched fixed-point noise suppressor on gfx950 (include/asp_nsx.h).
//
// One wave per stream: a workgroup is one wave, bin q, q + 64 and the bin-128 tail
// sit on lane q for every per-bin phase of nsx_core.h, cross-bin values are wave reductions, the 128 /
// 256-point FFT runs one butterfly per lane and step on a wave-private LDS row.  The stream's state
// (everything but the three histograms, which see three increments per frame and stay in HBM) and the
// frame's work arrays live in LDS for the F frames of a call.  Integer arithmetic: bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "nsx_core.h"

namespace aspnsx {
namespace {

constexpr int kWave = 64;
constexpr int kHistBegin = offsetof(AspNsxState, histLrt) / 4 * 4;  // word-aligned cut around the histograms
constexpr int kHistEnd = (offsetof(AspNsxState, dataBufHBFX) + 3) / 4 * 4;
static_assert(sizeof(AspNsxState) % 4 == 0, "state is copied by words");

__device__ inline void copy_words(uint32_t* dst, const uint32_t* src, int lane) {
  constexpr int a = kHistBegin / 4, b = kHistEnd / 4, n = sizeof(AspNsxState) / 4;
  for (int i = lane; i < a; i += kWave) dst[i] = src[i];
  for (int i = b + lane; i < n; i += kWave) dst[i] = src[i];
}

// low_in / low_out [F][S][n]; high_in / high_out [F][nb - 1][S][n]
__global__ void __launch_bounds__(kWave) nsx_frames_kernel(AspNsxState* __restrict__ st, const NsxTables* __restrict__ T,
                                                           int S, int F, int n, int nb, const int16_t* low_in,
                                                           const int16_t* high_in, int16_t* low_out,
                                                           int16_t* high_out) {
  __shared__ AspNsxState s;
  __shared__ NsxWork w;
  const int stream = blockIdx.x, lane = threadIdx.x;
  AspNsxState* g = st + stream;
  copy_words((uint32_t*)&s, (const uint32_t*)g, lane);
  // the bytes of the cut that are not histogram (alignment slack) travel too
  if (lane == 0) {
    unsigned char* d = (unsigned char*)&s;
    const unsigned char* c = (const unsigned char*)g;
    for (int i = kHistBegin; i < (int)offsetof(AspNsxState, histLrt); ++i) d[i] = c[i];
    for (int i = (int)offsetof(AspNsxState, dataBufHBFX); i < kHistEnd; ++i) d[i] = c[i];
  }
  wsync();
  const Lanes L{lane, kWave};
  for (int f = 0; f < F; ++f) {
    const int16_t* in[3];
    int16_t* out[3];
    in[0] = low_in + ((size_t)f * S + stream) * n;
    out[0] = low_out + ((size_t)f * S + stream) * n;
    for (int b = 1; b < nb; ++b) {
      const size_t off = (((size_t)f * (nb - 1) + (b - 1)) * S + stream) * n;
      in[b] = high_in + off;
      out[b] = high_out + off;
    }
    process_core(s, w, g->histLrt, in, nb, out, *T, L);
  }
  wsync();
  copy_words((uint32_t*)g, (const uint32_t*)&s, lane);
}

// op 0: Init(fs = arg); op 1: set_policy(mode = arg)
__global__ void __launch_bounds__(kWave) nsx_control_kernel(AspNsxState* __restrict__ st, int first, int count, int op,
                                                            int arg) {
  const int i = blockIdx.x * kWave + threadIdx.x;
  if (i >= count) return;
  if (op == 0)
    init_core(st[first + i], (uint32_t)arg);
  else
    set_policy_core(st[first + i], arg);
}

}  // namespace

hipError_t launch_frames(AspNsxState* st, const NsxTables* T, int S, int F, int n, int nb, const int16_t* low_in,
                         const int16_t* high_in, int16_t* low_out, int16_t* high_out, hipStream_t stream) {
  hipLaunchKernelGGL(nsx_frames_kernel, dim3(S), dim3(kWave), 0, stream, st, T, S, F, n, nb, low_in, high_in, low_out,
                     high_out);
  return hipGetLastError();
}

hipError_t launch_control(AspNsxState* st, int first, int count, int op, int arg, hipStream_t stream) {
  hipLaunchKernelGGL(nsx_control_kernel, dim3((count + kWave - 1) / kWave), dim3(kWave), 0, stream, st, first, count,
                     op, arg);
  return hipGetLastError();
}

}  // namespace aspnsx
