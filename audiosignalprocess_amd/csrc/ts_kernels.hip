// ts_kernels.hip -- the batched transient suppressor on gfx950 (include/asp_ts.h).
//
// One wave64 is one stream, a workgroup is one wave.  The stream's AspTsState (scalars,
// node histories, moment queues: 6.4 KB) is copied into LDS once per launch and written back once, across the F
// chunks; the work memory of ts_core.h (the transform buffer and the staging buffer, which the wavelet tree
// shares, magnitudes, the leaves' moments) is LDS as well.  in_buffer_, out_buffer_ and spectral_mean_ stay in
// HBM: every chunk reads and writes them once per channel, lanes on consecutive floats.  The channels of a
// stream run in sequence inside the wave: they share the detector's result and the seed.  The tables (window,
// FFT w, mean_factor_, the 32768 phases) are read through the cache.  Arithmetic: ts_core.h, bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "ts_core.h"

namespace aspts {
namespace {

constexpr int kWave = 64;
constexpr int kStateWords = sizeof(AspTsState) / 4;

// states [S]; bufs [S][stride]; data [F][S][C][L]; det [F][S][D] or NULL; ref [F][S][R] or NULL; present [F][S]
// or NULL; voice, keys [F][S]; results [F][S] or NULL; errors: incremented once per failed chunk
__global__ void __launch_bounds__(kWave)
    ts_suppress_kernel(TsConfig c, TsTables tb, AspTsState* __restrict__ states, float* __restrict__ bufs, size_t stride,
                       int S, int F, float* data, const float* det, const float* ref, int ref_len,
                       const uint8_t* present, const float* voice, const uint8_t* keys, int32_t* results, int* errors) {
  __shared__ AspTsState st;
  __shared__ TsWork w;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= S) return;
  const Grp g{lane, kWave};
  uint32_t* lds_words = reinterpret_cast<uint32_t*>(&st);
  uint32_t* hbm_words = reinterpret_cast<uint32_t*>(states + s);
  for (int i = lane; i < kStateWords; i += kWave) lds_words[i] = hbm_words[i];
  __syncthreads();
  float* in = bufs + (size_t)s * stride;
  float* out = in + (size_t)c.C * c.N;
  float* mean = out + (size_t)c.C * c.N;
  const size_t chunk = (size_t)c.C * c.L;
  for (int f = 0; f < F; ++f) {
    const size_t u = (size_t)f * S + s;
    float* d = data + u * chunk;
    const float* dd = det ? det + u * c.D : d;
    const float* rr = (ref && (!present || present[u])) ? ref + u * ref_len : nullptr;
    const int rc = suppress_chunk(c, tb, st, w, in, out, mean, d, dd, rr, ref_len, voice[u], keys[u], g);
    if (lane == 0) {
      if (results) results[u] = rc;
      if (rc) atomicAdd(errors, 1);
    }
    __syncthreads();
  }
  for (int i = lane; i < kStateWords; i += kWave) hbm_words[i] = lds_words[i];
}

}  // namespace

hipError_t launch_suppress(const TsConfig& c, const TsTables& tb, AspTsState* states, float* bufs, size_t stride, int S,
                           int F, float* data, const float* det, const float* ref, int ref_len, const uint8_t* present,
                           const float* voice, const uint8_t* keys, int32_t* results, int* errors, hipStream_t stream) {
  hipLaunchKernelGGL(ts_suppress_kernel, dim3(S), dim3(kWave), 0, stream, c, tb, states, bufs, stride, S, F, data, det,
                     ref, ref_len, present, voice, keys, results, errors);
  return hipGetLastError();
}

}  // namespace aspts
