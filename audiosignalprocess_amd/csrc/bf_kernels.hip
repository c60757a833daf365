// bf_kernels.hip -- the batched nonlinear beamformer on gfx950 (include/asp_bf.h).
//
// One wave64 is one stream, a workgroup is one wave.  The stream's whole state -- the
// AspBfState (1 KB: the scalars and the two saved mask rows), the Blocker's input buffer [M][384] and output
// buffer [384] -- is copied into LDS once per launch and written back once, across the F chunks; the M spectra
// and the output block are LDS as well (23.5 KB in all at M = 8).  The M forward transforms of a block run in
// sequence on the wave (ts_core.h's rdft); the mask stage then puts one bin on a lane in three passes (bins
// 0..63, 64..127, and bin 128 on lane 0), with the microphone vector of the bin in registers: the kernel is
// instantiated per microphone count so that every loop over microphones unrolls.  The batch-wide tables (bin-minor
// covariances, bf_layout.h) are read through the cache.  Arithmetic: bf_core.h, bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "bf_core.h"

namespace aspbf {
namespace {

constexpr int kWave = 64;
constexpr int kStateWords = sizeof(AspBfState) / 4;

template <int M>
struct BfLds {
  AspBfState st;
  float in[M * kBuf];
  float out[kBuf];
  BfWork<M> w;
};

// states [S]; bufs [S][(M + 1) * 384]; input [F][S][M][160]; high [F][S][M][160] or NULL; output [F][S][160];
// high_output [F][S][160] or NULL; present [F][S] or NULL
template <int M>
__global__ void __launch_bounds__(kWave)
    bf_chunks_kernel(BfParams p, BfTables tb, AspBfState* __restrict__ states, float* __restrict__ bufs, int S, int F,
                     const float* __restrict__ input, const float* __restrict__ high, float* __restrict__ output,
                     float* __restrict__ high_output, uint8_t* __restrict__ present) {
  __shared__ BfLds<M> l;
  const int s = blockIdx.x, lane = threadIdx.x;
  if (s >= S) return;
  const Grp g{lane, kWave};
  constexpr int kBufFloats = (M + 1) * kBuf;
  uint32_t* lds_words = reinterpret_cast<uint32_t*>(&l.st);
  uint32_t* hbm_words = reinterpret_cast<uint32_t*>(states + s);
  float* hbm_buf = bufs + (size_t)s * kBufFloats;
  float* lds_buf = l.in;  // in and out are adjacent: the stream's buffer array
  static_assert(offsetof(BfLds<M>, out) == offsetof(BfLds<M>, in) + sizeof(float) * M * kBuf, "in and out are one array");
  for (int i = lane; i < kStateWords; i += kWave) lds_words[i] = hbm_words[i];
  for (int i = lane; i < kBufFloats; i += kWave) lds_buf[i] = hbm_buf[i];
  __syncthreads();
  for (int f = 0; f < F; ++f) {
    const size_t u = (size_t)f * S + s;
    process_chunk<M>(p, tb, l.st, l.w, l.in, l.out, input + u * (M * kChunk), high ? high + u * (M * kChunk) : nullptr,
                     output + u * kChunk, high ? high_output + u * kChunk : nullptr, g);
    if (present && lane == 0) present[u] = (uint8_t)l.st.is_target_present;
  }
  __syncthreads();
  for (int i = lane; i < kStateWords; i += kWave) hbm_words[i] = lds_words[i];
  for (int i = lane; i < kBufFloats; i += kWave) hbm_buf[i] = lds_buf[i];
}

template <int M>
void launch(const BfParams& p, const BfTables& tb, AspBfState* states, float* bufs, int S, int F, const float* input,
            const float* high, float* output, float* high_output, uint8_t* present, hipStream_t stream) {
  hipLaunchKernelGGL(bf_chunks_kernel<M>, dim3(S), dim3(kWave), 0, stream, p, tb, states, bufs, S, F, input, high, output,
                     high_output, present);
}

}  // namespace

hipError_t launch_chunks(const BfParams& p, const BfTables& tb, AspBfState* states, float* bufs, int S, int F,
                         const float* input, const float* high, float* output, float* high_output, uint8_t* present,
                         hipStream_t stream) {
  switch (p.M) {
    case 2: launch<2>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    case 3: launch<3>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    case 4: launch<4>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    case 5: launch<5>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    case 6: launch<6>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    case 7: launch<7>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    case 8: launch<8>(p, tb, states, bufs, S, F, input, high, output, high_output, present, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace aspbf
