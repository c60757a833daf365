// splrs_kernels.hip -- the batched fixed-point resampler on gfx950 (include/asp_resampler.h).
//
// A unit is one channel of one stream.  kLanes = 16 lanes serve a unit, four units share a wave, a workgroup
// is one wave.  Per unit the wave keeps in LDS the 96 state words (read once and
// written once per call, across the F frames), two int16 buffers of 480 samples that the mode's chain
// ping-pongs between, and the block resamplers' int32 work buffer.  A Push is cut into pieces of 10 ms (one
// block of the mode's block loop): a piece is staged into LDS with consecutive lanes on consecutive
// samples, runs splrs_core.h's chain -- the all-pass branches of a by-2 stage on two lanes, the FIR stages
// and the combine steps across the 16 -- and is stored the same way.  The mode is uniform over the batch:
// the chain's switch is wave-uniform.  Integer arithmetic: bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "splrs_core.h"

namespace aspsplrs {
namespace {

constexpr int kWave = 64;
constexpr int kLanes = 16;
constexpr int kUnits = kWave / kLanes;   // units per wave

struct Lds {
  int32_t st[kUnits][kStateWords];
  int32_t w[kUnits][kWork];
  int16_t a[kUnits][kPieceMax], b[kUnits][kPieceMax];
};

// state [U][96]; in [F][U / ch][len * ch], out [F][U / ch][olen * ch]: channel c of a stream is every ch-th
// sample from c (len, olen: per channel)
__global__ void __launch_bounds__(kWave) splrs_push_kernel(int32_t* __restrict__ state, const int16_t* __restrict__ in,
                                                           int16_t* __restrict__ out, int U, int ch, int mode, int len,
                                                           int olen, int F) {
  __shared__ Lds lds;
  const int g = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  const int unit = blockIdx.x * kUnits + g;
  const bool valid = unit < U;
  const int u = valid ? unit : U - 1;   // a unit past the end computes on a copy and stores nothing
  int32_t* st = lds.st[g];
  for (int i = lane; i < kStateWords; i += kLanes) st[i] = state[(size_t)u * kStateWords + i];
  wsync();
  const int S = U / ch, s = u / ch, c = u - s * ch;
  const int piece = kChain[mode].piece;
  for (int f = 0; f < F; ++f) {
    const int16_t* src = in + ((size_t)f * S + s) * len * ch + c;
    int16_t* dst = out + ((size_t)f * S + s) * olen * ch + c;
    int done = 0;
    for (int off = 0; off < len; off += piece) {
      const int n = len - off < piece ? len - off : piece;
      for (int i = lane; i < n; i += kLanes) lds.a[g][i] = src[(size_t)(off + i) * ch];
      wsync();
      int16_t* res;
      const int m = push_piece<kLanes>(mode, st, lds.a[g], n, lds.b[g], lds.w[g], lane, &res);
      wsync();
      if (valid)
        for (int i = lane; i < m; i += kLanes) dst[(size_t)(done + i) * ch] = res[i];
      done += m;
      wsync();   // the next piece's staging overwrites the buffers
    }
  }
  if (valid)
    for (int i = lane; i < kStateWords; i += kLanes) state[(size_t)unit * kStateWords + i] = st[i];
}

}  // namespace

hipError_t launch_push(int32_t* state, const int16_t* in, int16_t* out, int U, int ch, int mode, int len, int olen,
                       int F, hipStream_t stream) {
  hipLaunchKernelGGL(splrs_push_kernel, dim3((U + kUnits - 1) / kUnits), dim3(kWave), 0, stream, state, in, out, U, ch,
                     mode, len, olen, F);
  return hipGetLastError();
}

}  // namespace aspsplrs
