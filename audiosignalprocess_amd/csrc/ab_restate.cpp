// ab_restate.cpp -- the CPU build of ab_core.h and sinc_plan.h, for the tests only (lib/libab_restate.so; not part
// of libasp_amd.so, which has no CPU path).  The same arithmetic the kernels run and the same plan the host hands
// them, one channel at a time: tests/test_ab_host.py holds it to the golden on machines without a GPU.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ab_core.h"
#include "sinc_plan.h"

using namespace aspab;
using namespace aspsinc;

namespace {
struct Resampler {
  SincHost h;
  std::vector<float> buf;  // SincResampler::input_buffer_
};

struct Row {
  const float* k;
  Quad operator()(int c) const { return Quad{k[4 * c], k[4 * c + 1], k[4 * c + 2], k[4 * c + 3]}; }
};
}  // namespace

extern "C" {

void AbRestate_FloatToFloatS16(const float* src, int n, float* dst) {
  for (int i = 0; i < n; ++i) dst[i] = float_to_float_s16(src[i]);
}
void AbRestate_FloatS16ToFloat(const float* src, int n, float* dst) {
  for (int i = 0; i < n; ++i) dst[i] = float_s16_to_float(src[i]);
}
void AbRestate_FloatS16ToS16(const float* src, int n, int16_t* dst) {
  for (int i = 0; i < n; ++i) dst[i] = float_s16_to_s16(src[i]);
}
void AbRestate_S16ToFloatS16(const int16_t* src, int n, float* dst) {
  for (int i = 0; i < n; ++i) dst[i] = s16_to_float_s16(src[i]);
}
void AbRestate_StereoToMonoS16(const int16_t* l, const int16_t* r, int n, int16_t* dst) {
  for (int i = 0; i < n; ++i) dst[i] = stereo_to_mono(l[i], r[i]);
}
void AbRestate_StereoToMonoFloat(const float* l, const float* r, int n, float* dst) {
  for (int i = 0; i < n; ++i) dst[i] = stereo_to_mono(l[i], r[i]);
}

// PushSincResampler(source_frames, destination_frames), float path
void* AbRestate_ResamplerCreate(int source_frames, int destination_frames) {
  if (source_frames <= kKernelSize || destination_frames <= 0) return nullptr;
  Resampler* r = new Resampler;
  init_push(&r->h, source_frames, destination_frames);
  r->buf.assign(r->h.buf_len, 0.f);
  return r;
}
void AbRestate_ResamplerFree(void* h) { delete (Resampler*)h; }
float* AbRestate_ResamplerBuffer(void* h) { return ((Resampler*)h)->buf.data(); }
int AbRestate_ResamplerBufferLength(void* h) { return ((Resampler*)h)->h.buf_len; }
const float* AbRestate_ResamplerKernel(void* h) { return ((Resampler*)h)->h.kernel_host.data(); }

// PushSincResampler::Resample(const float*, ...): the plan of sinc_plan.h walked the way ab_copy_kernel walks it
int AbRestate_Resample(void* h, const float* in, float* out) {
  Resampler* r = (Resampler*)h;
  SincPlan plan;
  memset(&plan, 0, sizeof plan);
  if (!plan_push(&r->h, &plan)) return -1;
  float* buf = r->buf.data();
  const float* ktab = r->h.kernel_host.data();
  for (int s = 0; s < plan.nseg; ++s) {
    const SincSeg& sg = plan.seg[s];
    if (sg.load != 0) {
      if (sg.shift) memmove(buf, buf + sg.r3, kKernelSize * sizeof(float));
      for (int i = 0; i < r->h.src; ++i) buf[sg.r0 + i] = sg.load == 2 ? in[i] : 0.f;
    }
    for (int m = sg.out_begin; m < sg.out_end; ++m) {
      const OutDesc& d = r->h.desc_host[m];
      const float* k1 = ktab + d.offset_idx * kKernelSize;
      const float v = convolve32(buf + d.source_idx, Row{k1}, Row{k1 + kKernelSize}, d.f1, d.f2);
      if (d.dest >= 0) out[d.dest] = v;
    }
  }
  return r->h.dst;
}
}
