// sinc_plan.h -- the host arithmetic of SincResampler / PushSincResampler that depends only on the call
// sequence: region bookkeeping, the kernel table, and Resample() as a plan of segments and per-output
// descriptors (sinc_layout.h).  Shared by sinc_api.hip (int16 I/O) and ab_api.hip (the float path of
// AudioBuffer::CopyFrom / CopyTo).  Host-only, header-only.
//
// P is a position record with the members of SincPos below plus `src` (request frames), `kernel_host` and
// `desc_host`; AspSincBatch carries them directly, the audio buffer through SincHost.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "sinc_layout.h"

namespace aspsinc {

// SincResampler / PushSincResampler position state (identical for every channel of a batch)
struct SincPos {
  double vsi;  // virtual_source_idx_
  int32_t r0, r3, r4, block_size;
  int32_t primed, first_pass;
};

struct SincHost {
  int src = 0, dst = 0, buf_len = 0;
  double ratio = 0, vsi = 0;
  int r0 = 0, r3 = 0, r4 = 0, block_size = 0;
  bool primed = false, first_pass = true;
  std::vector<float> kernel_host;
  std::vector<OutDesc> desc_host;
};

template <class P>
inline SincPos get_pos(const P* b) {
  return SincPos{b->vsi, b->r0, b->r3, b->r4, b->block_size, b->primed ? 1 : 0, b->first_pass ? 1 : 0};
}

template <class P>
inline void set_pos(P* b, const SincPos& p) {
  b->vsi = p.vsi;
  b->r0 = p.r0;
  b->r3 = p.r3;
  b->r4 = p.r4;
  b->block_size = p.block_size;
  b->primed = p.primed != 0;
  b->first_pass = p.first_pass != 0;
}

inline bool same_pos(const SincPos& a, const SincPos& b) {
  return a.vsi == b.vsi && a.r0 == b.r0 && a.r3 == b.r3 && a.r4 == b.r4 && a.block_size == b.block_size &&
         a.primed == b.primed && a.first_pass == b.first_pass;
}

template <class P>
inline void update_regions(P* b, bool second_load) {  // sinc_resampler.cc:190-199
  b->r0 = second_load ? kKernelSize : kKernelSize / 2;
  b->r3 = b->r0 + b->src - kKernelSize;
  b->r4 = b->r0 + b->src - kKernelSize / 2;
  b->block_size = b->r4 - kKernelSize / 2;
}

// NOTE: C++ translation unit; libm calls take explicit doubles so the arithmetic is the reference's.
template <class P>
inline void init_kernel(P* b) {  // sinc_resampler.cc:201-232, 88-101
  const double kAlpha = 0.16;
  const double kA0 = 0.5 * (1.0 - kAlpha), kA1 = 0.5, kA2 = 0.5 * kAlpha;
  double sinc_scale_factor = b->ratio > 1.0 ? 1.0 / b->ratio : 1.0;
  sinc_scale_factor *= 0.9;
  b->kernel_host.assign((size_t)kKernelSize * (kKernelOffsetCount + 1), 0.f);
  for (int offset_idx = 0; offset_idx <= kKernelOffsetCount; ++offset_idx) {
    const float subsample_offset = static_cast<float>(offset_idx) / kKernelOffsetCount;
    for (int i = 0; i < kKernelSize; ++i) {
      const int idx = i + offset_idx * kKernelSize;
      const float pre_sinc = static_cast<float>(M_PI * (double)(i - kKernelSize / 2 - subsample_offset));
      const float x = (i - subsample_offset) / kKernelSize;
      const float window = static_cast<float>(kA0 - kA1 * cos(2.0 * M_PI * (double)x) + kA2 * cos(4.0 * M_PI * (double)x));
      b->kernel_host[idx] = static_cast<float>(
          (double)window * ((pre_sinc == 0) ? sinc_scale_factor
                                            : (sin(sinc_scale_factor * (double)pre_sinc) / (double)pre_sinc)));
    }
  }
}

// SincResampler::Resample(frames, destination) as a plan: appends segments / descriptors.
// dest_base >= 0: outputs land at dest_base + k of the caller's buffer; < 0: discarded.
// Returns false when the plan would need more than its six segments.
template <class P>
inline bool plan_resample(P* b, int frames, int dest_base, SincPlan* plan) {
  int remaining = frames, produced = 0;
  auto open_seg = [&](int load, int shift) -> SincSeg* {
    if (plan->nseg >= 6) return nullptr;
    SincSeg* sg = &plan->seg[plan->nseg++];
    sg->load = load;
    sg->shift = shift;
    sg->r0 = b->r0;
    sg->r3 = b->r3;
    sg->out_begin = sg->out_end = (int)b->desc_host.size();
    return sg;
  };
  SincSeg* cur = nullptr;
  if (!b->primed && remaining) {  // read_cb_->Run(request_frames_, r0_)
    cur = open_seg(b->first_pass ? 1 : 2, 0);
    if (!cur) return false;
    b->first_pass = false;
    b->primed = true;
  }
  if (!cur) {
    cur = open_seg(0, 0);
    if (!cur) return false;
  }
  while (remaining) {
    for (int i = (int)ceil((b->block_size - b->vsi) / b->ratio); i > 0; --i) {
      const int source_idx = (int)b->vsi;
      const double subsample_remainder = b->vsi - source_idx;
      const double virtual_offset_idx = subsample_remainder * kKernelOffsetCount;
      const int offset_idx = (int)virtual_offset_idx;
      const double factor = virtual_offset_idx - offset_idx;
      OutDesc d;
      d.source_idx = source_idx;
      d.offset_idx = offset_idx;
      d.f1 = static_cast<float>(1.0 - factor);
      d.f2 = static_cast<float>(factor);
      d.dest = dest_base >= 0 ? dest_base + produced : -1;
      b->desc_host.push_back(d);
      cur->out_end = (int)b->desc_host.size();
      ++produced;
      b->vsi += b->ratio;
      if (!--remaining) return true;
    }
    b->vsi -= b->block_size;
    const int r3_before = b->r3;
    if (b->r0 == kKernelSize / 2) update_regions(b, true);
    const int load = b->first_pass ? 1 : 2;
    b->first_pass = false;
    cur = open_seg(load, 1);
    if (!cur) return false;
    cur->r3 = r3_before;  // the shift reads the region of the block just consumed
  }
  return true;
}

// PushSincResampler(source_frames, destination_frames): push_sinc_resampler.cc:19, Flush (sinc_resampler.cc:335-341)
template <class P>
inline void init_push(P* b, int source_frames, int destination_frames) {
  b->src = source_frames;
  b->dst = destination_frames;
  b->buf_len = source_frames + kKernelSize;
  b->ratio = source_frames * 1.0 / destination_frames;
  b->vsi = 0;
  b->primed = false;
  b->first_pass = true;
  update_regions(b, false);
  init_kernel(b);
}

// PushSincResampler::Resample (push_sinc_resampler.cc:47-78): a priming pass on the first call, then the call's
// destination_frames outputs.  Clears and fills b->desc_host.
template <class P>
inline bool plan_push(P* b, SincPlan* plan) {
  plan->nseg = 0;
  b->desc_host.clear();
  if (b->first_pass && !plan_resample(b, (int)(b->block_size / b->ratio), -1, plan)) return false;  // ChunkSize()
  return plan_resample(b, b->dst, 0, plan);
}

}  // namespace aspsinc
