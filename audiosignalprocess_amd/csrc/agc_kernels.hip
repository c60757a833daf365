// agc_kernels.hip -- the batched legacy gain control on gfx950 (include/asp_agc.h).
//
// kLanes = 16 lanes serve a stream (the 16-sample sub-frame at 16 kHz and up), four streams share a wave, a
// workgroup is one wave.  Per stream the wave keeps in LDS the AspAgcState (read once
// and written once per call, across the F frames) and the frame's AgcWork: the bands being worked on, the
// far end, the sub-frame envelope and gains.  A frame is staged with consecutive lanes on consecutive
// samples, runs agc_core.h's frame_core -- per-sample work across the 16 lanes, the three AgcVad chains as one
// pass on lanes 0..2, AddMic's decimator as a second pass on lane 3, the capacitor recurrences and
// ProcessAnalog on lane 0, the limiter one sub-frame per lane -- and is stored the same way.  Streams of a wave may differ in mode and
// rate family member; their branches diverge per 16-lane group, and every cross-lane step stays inside a
// group.  Integer arithmetic: bit-exact.
#include <hip/hip_runtime.h>

#include <stddef.h>

#include "agc_core.h"

namespace aspagc {
namespace {

constexpr int kWave = 64;
constexpr int kLanes = 16;
constexpr int kUnits = kWave / kLanes;   // streams per wave
constexpr int kStateWords = sizeof(AspAgcState) / 4;
static_assert(sizeof(AspAgcState) % 4 == 0, "state is copied by words");

struct Lds {
  AspAgcState st[kUnits];
  AgcWork w[kUnits];
};

}  // namespace

struct FrameArgs {
  AspAgcState* state;        // [S]
  int32_t* level;            // [S]: the stored microphone levels
  int S, F, n, nb, ops;
  const int16_t *far, *low_in, *high_in;
  int16_t *low_out, *high_out;
  const int32_t* level_in;   // [F][S] or NULL: chained from `level`
  const int16_t* echo;       // [F][S] or NULL
  int32_t *level_out, *vm_out;   // [F][S] or NULL: Process's outMicLevel, VirtualMic's micLevelOut
  uint8_t* saturation;       // [F][S] or NULL
  int32_t* rc;               // [F][S]
};

namespace {

__global__ void __launch_bounds__(kWave) agc_frames_kernel(FrameArgs a) {
  __shared__ Lds lds;
  const int u = threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  const int stream = blockIdx.x * kUnits + u;
  if (stream >= a.S) return;   // a whole group leaves; the groups of a wave never wait for one another
  AspAgcState& s = lds.st[u];
  AgcWork& w = lds.w[u];
  const Grp<kLanes> g{lane};
  {
    const uint32_t* src = (const uint32_t*)(a.state + stream);
    uint32_t* dst = (uint32_t*)&s;
    for (int i = lane; i < kStateWords; i += kLanes) dst[i] = src[i];
  }
  wsync();
  const int S = a.S, n = a.n, nb = a.nb;
  const bool audio = (a.ops & (kOpAddMic | kOpVirtualMic | kOpProcess | kOpByMode)) != 0;
  int32_t lv = a.level[stream];   // the chained level: kept up to date on lane 0 only, where frame_core reads level_in
  for (int f = 0; f < a.F; ++f) {
    const size_t fs = (size_t)f * S + stream;
    if (audio) {
      const int16_t* lo = a.low_in + fs * n;
      for (int i = lane; i < n; i += kLanes) w.x[0][i] = lo[i];
      for (int b = 1; b < nb; ++b) {
        const int16_t* hi = a.high_in + (((size_t)f * (nb - 1) + (b - 1)) * S + stream) * n;
        for (int i = lane; i < n; i += kLanes) w.x[b][i] = hi[i];
      }
    }
    if (a.ops & kOpFar) {
      const int16_t* fa = a.far + fs * n;
      for (int i = lane; i < n; i += kLanes) w.far[i] = fa[i];
    }
    wsync();
    FrameIo io;
    io.level_in = a.level_in ? a.level_in[fs] : lv;
    io.echo = a.echo ? a.echo[fs] : (int16_t)0;
    io.vm_level = io.level_out = io.level_in;
    io.saturation = 0;
    io.rc = 0;
    frame_core<kLanes>(s, w, a.ops, nb, n, io, g);
    wsync();
    if (audio) {
      int16_t* lo = a.low_out + fs * n;
      for (int i = lane; i < n; i += kLanes) lo[i] = w.x[0][i];
      for (int b = 1; b < nb; ++b) {
        int16_t* hi = a.high_out + (((size_t)f * (nb - 1) + (b - 1)) * S + stream) * n;
        for (int i = lane; i < n; i += kLanes) hi[i] = w.x[b][i];
      }
    }
    if (lane == 0) {
      a.rc[fs] = io.rc;
      if (a.vm_out) a.vm_out[fs] = io.vm_level;
      if (a.ops & kOpProcess) {
        if (a.level_out) a.level_out[fs] = io.level_out;
        if (a.saturation) a.saturation[fs] = io.saturation;
        // the chain: an adaptive-digital stream keeps its static physical level
        if (s.agcMode != kAgcModeAdaptiveDigital) lv = io.level_out;
      }
    }
    wsync();   // the next frame's staging overwrites the buffers
  }
  {
    uint32_t* dst = (uint32_t*)(a.state + stream);
    const uint32_t* src = (const uint32_t*)&s;
    for (int i = lane; i < kStateWords; i += kLanes) dst[i] = src[i];
  }
  if (lane == 0 && !a.level_in && (a.ops & kOpByMode)) a.level[stream] = lv;
}

}  // namespace

hipError_t launch_frames(const FrameArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(agc_frames_kernel, dim3((a.S + kUnits - 1) / kUnits), dim3(kWave), 0, stream, a);
  return hipGetLastError();
}

}  // namespace aspagc
