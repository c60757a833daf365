// aecm_kernels.hip -- the batched mobile echo canceller on gfx950 (include/asp_aecm.h).
//
// One lane per stream.  A call of F frames runs, per lane, "BufferFarend, then
// Process" for each frame in time order over the stream's AspAecmState and AecmWork in HBM
// (aecm_core.h); the lanes of a wave are independent streams.  Integer arithmetic throughout: bit-exact
// with the reference.
#include <hip/hip_runtime.h>

#include "aecm_core.h"

namespace aspaecm {
namespace {

constexpr int kBlock = 64;

__global__ void __launch_bounds__(kBlock) aecm_frames_kernel(AspAecmState* __restrict__ st, AecmWork* __restrict__ wk,
                                                             const AecmTables* __restrict__ T, int S, int F, int n,
                                                             const int16_t* far, const int16_t* near,
                                                             const int16_t* clean, int16_t* out,
                                                             const int16_t* __restrict__ ms) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= S) return;
  AspAecmState& state = st[s];
  AecmWork& work = wk[s];
  for (int f = 0; f < F; ++f) {
    const size_t off = ((size_t)f * S + s) * n;
    if (far) buffer_farend(state, far + off, n);
    if (near) process(state, work, near + off, clean ? clean + off : nullptr, out + off, n, ms[(size_t)f * S + s], *T);
  }
}

// op 0: Init(fs = arg); op 1: set_config(cng = arg & 1, echo = (arg >> 1) - 1; -1: cngMode only);
// op 2: InitEchoPath(path)
__global__ void __launch_bounds__(kBlock) aecm_control_kernel(AspAecmState* __restrict__ st,
                                                              const AecmTables* __restrict__ T, int first, int count,
                                                              int op, int arg, const int16_t* path) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  AspAecmState& state = st[first + i];
  if (op == 0)
    init_instance(state, arg, *T);
  else if (op == 1 && (arg >> 1) == 0)
    state.cngMode = (int16_t)(arg & 1);
  else if (op == 1)
    set_config(state, arg & 1, (arg >> 1) - 1);
  else
    init_echo_path_core(state, path);
}

}  // namespace

hipError_t launch_frames(AspAecmState* st, AecmWork* wk, const AecmTables* T, int S, int F, int n,
                         const int16_t* far, const int16_t* near, const int16_t* clean, int16_t* out,
                         const int16_t* ms, hipStream_t stream) {
  hipLaunchKernelGGL(aecm_frames_kernel, dim3((S + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, st, wk, T, S, F,
                     n, far, near, clean, out, ms);
  return hipGetLastError();
}

hipError_t launch_control(AspAecmState* st, const AecmTables* T, int first, int count, int op, int arg,
                          const int16_t* path, hipStream_t stream) {
  hipLaunchKernelGGL(aecm_control_kernel, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, st, T,
                     first, count, op, arg, path);
  return hipGetLastError();
}

}  // namespace aspaecm
