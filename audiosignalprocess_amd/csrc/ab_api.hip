// ab_api.hip -- host side of include/asp_audio_buffer.h: the batch handle (device storage of ab_layout.h), the
// reference's valid-flag state machine (IFChannelBuffer, mixed_low_pass_valid_, reference_copied_) and the
// resamplers' position arithmetic (sinc_plan.h), both of which depend only on the call sequence and so run once per
// batch here, argument checks, staging for host-memory callers, the checkpoint.  The band split is AspSplitBatch
// (qmf_api.hip) on the batch's stream.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "ab_layout.h"
#include "api_common.h"
#include "asp_split.h"

using namespace aspab;
using namespace aspsinc;

namespace aspab {
hipError_t launch_deinterleave(const InterleaveArgs& a, hipStream_t s);
hipError_t launch_interleave(const InterleaveArgs& a, hipStream_t s);
hipError_t launch_refresh_i(const RefreshIArgs& a, hipStream_t s);
hipError_t launch_refresh_f(const RefreshFArgs& a, hipStream_t s);
hipError_t launch_copy(const CopyArgs& a, bool from, hipStream_t s);
}  // namespace aspab

#define ab_fail(...) asp_fail("asp_audio_buffer", __VA_ARGS__)
#define AB_TRY(x) ASP_TRY("asp_audio_buffer", x)

namespace {

// IFChannelBuffer's two flags
struct Pair {
  bool iv = true, fv = true;
};

// The descriptor tables of a resampler: a ring of slots on the device, each with a pinned host twin and the event
// of the last kernel that read it, as in sinc_api.hip (a call whose table differs from the previous one takes the
// next slot: no stream synchronisation on the way).
struct DescRing {
  static constexpr int kSlots = 4;
  OutDesc *dev = nullptr, *pinned = nullptr;
  hipEvent_t ev[kSlots] = {};
  size_t cap = 0;
  int slot = 0;
  std::vector<OutDesc> last;

  hipError_t init(size_t capacity) {
    cap = capacity;
    hipError_t e = hipMalloc((void**)&dev, kSlots * cap * sizeof(OutDesc));
    if (e == hipSuccess) e = hipHostMalloc((void**)&pinned, kSlots * cap * sizeof(OutDesc));
    for (int i = 0; i < kSlots && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    return e;
  }
  void release() {
    if (dev) (void)hipFree(dev);
    if (pinned) (void)hipHostFree(pinned);
    for (int i = 0; i < kSlots; ++i)
      if (ev[i]) (void)hipEventDestroy(ev[i]);
  }
  hipError_t upload(const std::vector<OutDesc>& d, hipStream_t s, const OutDesc** out) {
    if (d.size() > cap) return hipErrorInvalidValue;
    if (last.size() != d.size() || memcmp(last.data(), d.data(), d.size() * sizeof(OutDesc)) != 0) {
      slot = (slot + 1) % kSlots;
      hipError_t e = hipEventSynchronize(ev[slot]);
      if (e != hipSuccess) return e;
      memcpy(pinned + slot * cap, d.data(), d.size() * sizeof(OutDesc));
      e = hipMemcpyAsync(dev + slot * cap, pinned + slot * cap, d.size() * sizeof(OutDesc), hipMemcpyHostToDevice, s);
      if (e != hipSuccess) return e;
      last = d;
    }
    *out = dev + slot * cap;
    return hipSuccess;
  }
  hipError_t mark(hipStream_t s) { return hipEventRecord(ev[slot], s); }
};

bool io_length(int n) { return n == 80 || n == 160 || n == 320 || n == 441 || n == 480; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

struct AspAudioBufferBatch {
  int S = 0, Pin = 0, Cin = 0, P = 0, Cp = 0, Pout = 0, device = 0;
  int nb = 1, ns = 0;        // num_bands_, samples_per_split_channel_
  bool has_bands = false;    // split_channels_ is not empty
  // per batch: what depends on the call sequence only
  int num_channels = 0;
  bool mixed_valid = false, ref_copied = false;
  Pair ch, band[ASP_AB_MAX_BANDS];
  const float* keyboard = nullptr;
  std::vector<int32_t> activity;  // [S]
  SincHost in_res, out_res[2];
  // device
  hipStream_t own_stream = nullptr, stream = nullptr;
  int16_t *ch_i = nullptr, *band_i = nullptr, *mixed = nullptr, *ref = nullptr;
  float *ch_f = nullptr, *band_f = nullptr;
  float *rs_in = nullptr, *rs_out = nullptr, *kt_in = nullptr, *kt_out = nullptr;
  DescRing ring_in, ring_out;
  AspSplitBatch* split = nullptr;
  AspStage s_io;  // staging for host-memory callers

  size_t U() const { return (size_t)S * Cp; }
};

namespace {

// the buffers split_bands() walks: the bands, or the full band as band 0 of a buffer without bands
struct BandSet {
  int16_t* bi;
  float* bf;
  int nb, ns;
  Pair* pair[ASP_AB_MAX_BANDS];
};

BandSet bands_of(AspAudioBufferBatch* b) {
  BandSet t{};
  if (b->has_bands) {
    t.bi = b->band_i;
    t.bf = b->band_f;
    t.nb = b->nb;
    t.ns = kBandSamples;
    for (int k = 0; k < b->nb; ++k) t.pair[k] = &b->band[k];
  } else {
    t.bi = b->ch_i;
    t.bf = b->ch_f;
    t.nb = 1;
    t.ns = b->P;
    t.pair[0] = &b->ch;
  }
  return t;
}

// RefreshI on every stale int16 side of the set (ibuf_const of each), with the consumers of band 0 in the same
// launch; launches nothing when nothing is stale and nothing is consumed
int refresh_set(AspAudioBufferBatch* b, int16_t* mixed, int16_t* ref) {
  BandSet t = bands_of(b);
  int mask = 0;
  for (int k = 0; k < t.nb; ++k)
    if (!t.pair[k]->iv) mask |= 1 << k;
  if (!mask && !mixed && !ref) return ASP_OK;
  RefreshIArgs a{t.bi, t.bf, mixed, ref, b->S, b->Cp, t.ns, t.nb, mask};
  AB_TRY(launch_refresh_i(a, b->stream));
  for (int k = 0; k < t.nb; ++k) t.pair[k]->iv = true;
  return ASP_OK;
}

// IFChannelBuffer::ibuf / ibuf_const / fbuf / fbuf_const of channels_ (band < 0) or a band
int touch(AspAudioBufferBatch* b, int band, bool want_float, bool is_const) {
  Pair& p = band < 0 ? b->ch : b->band[band];
  const int n = band < 0 ? b->P : kBandSamples;
  const size_t len = b->U() * n, off = band < 0 ? 0 : (size_t)band * len;
  int16_t* bi = (band < 0 ? b->ch_i : b->band_i) + off;
  float* bf = (band < 0 ? b->ch_f : b->band_f) + off;
  if (want_float) {
    if (!p.fv) {
      AB_TRY(launch_refresh_f(RefreshFArgs{bi, bf, (int)(len / kGroup)}, b->stream));
      p.fv = true;
    }
    if (!is_const) p.iv = false;
  } else {
    if (!p.iv) {
      AB_TRY(launch_refresh_i(RefreshIArgs{bi, bf, nullptr, nullptr, b->S, b->Cp, n, 1, 1}, b->stream));
      p.iv = true;
    }
    if (!is_const) p.fv = false;
  }
  return ASP_OK;
}

// split_channels / _const / _f / _const_f (audio_buffer.cc:249-322); band < 0: channels / ..._f
void* view(AspAudioBufferBatch* b, int band, bool want_float, bool is_const, const char* who) {
  if (!b) {
    ab_fail(ASP_ERR_PARAM, who);
    return nullptr;
  }
  AspDeviceScope dev_scope_;
  if (dev_scope_.select(b->device) != hipSuccess) {
    ab_fail(ASP_ERR_HIP, who);
    return nullptr;
  }
  if (!is_const) b->mixed_valid = false;
  int which = band;
  if (band >= 0) {
    if (b->has_bands) {
      if (band >= b->nb) return nullptr;
    } else {
      if (band != 0) return nullptr;
      which = -1;
    }
  }
  if (touch(b, which, want_float, is_const) != ASP_OK) return nullptr;
  const size_t off = which < 0 ? 0 : (size_t)which * b->U() * kBandSamples;
  if (want_float) return (which < 0 ? b->ch_f : b->band_f) + off;
  return (which < 0 ? b->ch_i : b->band_i) + off;
}

void init_for_new_data(AspAudioBufferBatch* b) {  // AudioBuffer::InitForNewData
  b->keyboard = nullptr;
  b->mixed_valid = false;
  b->ref_copied = false;
  b->activity.assign(b->S, ASP_AB_VAD_UNKNOWN);
  b->num_channels = b->Cp;
}

bool good_mem(int mem) { return mem == ASP_MEM_HOST || mem == ASP_MEM_DEVICE; }

AbRecord record_of(const AspAudioBufferBatch* b) {
  AbRecord r;
  memset(&r, 0, sizeof r);
  r.magic = kRecordMagic;
  const int g[5] = {b->Pin, b->Cin, b->P, b->Cp, b->Pout};
  memcpy(r.geometry, g, sizeof g);
  r.num_channels = b->num_channels;
  r.ch_ivalid = b->ch.iv;
  r.ch_fvalid = b->ch.fv;
  for (int k = 0; k < ASP_AB_MAX_BANDS; ++k) {
    r.band_ivalid[k] = b->band[k].iv;
    r.band_fvalid[k] = b->band[k].fv;
  }
  r.mixed_valid = b->mixed_valid;
  r.reference_copied = b->ref_copied;
  if (b->rs_in) r.in_pos = get_pos(&b->in_res);
  if (b->rs_out)
    for (int c = 0; c < b->Cp; ++c) r.out_pos[c] = get_pos(&b->out_res[c]);
  return r;
}

}  // namespace

extern "C" {

int AspAudioBufferBatch_Free(AspAudioBufferBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->split) AspSplitBatch_Free(b->split);
  void* bufs[] = {b->ch_i, b->band_i, b->mixed, b->ref, b->ch_f, b->band_f, b->rs_in, b->rs_out, b->kt_in, b->kt_out};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  b->ring_in.release();
  b->ring_out.release();
  b->s_io.release();
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspAudioBufferBatch_Create(AspAudioBufferBatch** out, int num_streams, int input_samples, int num_input_channels,
                               int proc_samples, int num_proc_channels, int output_samples, int device) {
  if (!out) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Create: NULL out");
  *out = nullptr;
  if (num_streams < 1 || (int64_t)num_streams * 2 * 512 > INT32_MAX / 4)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Create: num_streams < 1 or too large");
  if (num_input_channels < 1 || num_input_channels > 2)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Create: num_input_channels is not 1 or 2");
  if (num_proc_channels < 1 || num_proc_channels > num_input_channels)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Create: num_proc_channels < 1 or > num_input_channels");
  if (!io_length(input_samples) || !io_length(output_samples))
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Create: input / output samples not 80, 160, 320, 441 or 480");
  if (!io_length(proc_samples) || proc_samples == 441)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Create: proc_samples not 80, 160, 320 or 480");
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_audio_buffer", device, ASP_ERR_NO_DEVICE,
                                 "AspAudioBufferBatch_Create: no HIP device (the audio buffer has no CPU path)"))
    return rc;
  AspAudioBufferBatch* b = new AspAudioBufferBatch;
  b->S = num_streams;
  b->Pin = input_samples;
  b->Cin = num_input_channels;
  b->P = proc_samples;
  b->Cp = num_proc_channels;
  b->Pout = output_samples;
  b->device = device;
  b->num_channels = b->Cp;
  b->has_bands = proc_samples == 320 || proc_samples == 480;
  b->ns = b->has_bands ? kBandSamples : proc_samples;
  b->nb = b->has_bands ? proc_samples / kBandSamples : 1;
  b->activity.assign(b->S, ASP_AB_VAD_UNKNOWN);
  const size_t U = b->U();
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  b->stream = b->own_stream;
  auto zalloc = [&](void** p, size_t bytes) {
    if (e == hipSuccess) e = hipMalloc(p, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(*p, 0, bytes, b->stream);
  };
  zalloc((void**)&b->ch_i, U * b->P * sizeof(int16_t));
  zalloc((void**)&b->ch_f, U * b->P * sizeof(float));
  if (b->has_bands) {
    zalloc((void**)&b->band_i, b->nb * U * kBandSamples * sizeof(int16_t));
    zalloc((void**)&b->band_f, b->nb * U * kBandSamples * sizeof(float));
  }
  zalloc((void**)&b->mixed, (size_t)b->S * b->ns * sizeof(int16_t));
  zalloc((void**)&b->ref, U * b->ns * sizeof(int16_t));
  if (b->Pin != b->P) {
    init_push(&b->in_res, b->Pin, b->P);
    zalloc((void**)&b->rs_in, U * b->in_res.buf_len * sizeof(float));
    zalloc((void**)&b->kt_in, b->in_res.kernel_host.size() * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpyAsync(b->kt_in, b->in_res.kernel_host.data(), b->in_res.kernel_host.size() * sizeof(float),
                         hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = b->ring_in.init((size_t)b->P * 2 + 64);
  }
  if (b->Pout != b->P) {
    for (int c = 0; c < b->Cp; ++c) init_push(&b->out_res[c], b->P, b->Pout);
    zalloc((void**)&b->rs_out, U * b->out_res[0].buf_len * sizeof(float));
    zalloc((void**)&b->kt_out, b->out_res[0].kernel_host.size() * sizeof(float));
    if (e == hipSuccess)
      e = hipMemcpyAsync(b->kt_out, b->out_res[0].kernel_host.data(), b->out_res[0].kernel_host.size() * sizeof(float),
                         hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess) e = b->ring_out.init(((size_t)b->Pout * 2 + 64) * b->Cp);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  int rc = e == hipSuccess ? ASP_OK : ab_fail(ASP_ERR_HIP, "AspAudioBufferBatch_Create", e);
  if (rc == ASP_OK && b->has_bands) {
    rc = AspSplitBatch_Create(&b->split, (int)U, b->nb, device);
    if (rc == ASP_OK) rc = AspSplitBatch_SetStream(b->split, b->stream);
  }
  if (rc != ASP_OK) {
    AspAudioBufferBatch_Free(b);
    return rc;
  }
  *out = b;
  return ASP_OK;
}

int AspAudioBufferBatch_num_streams(const AspAudioBufferBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

// ------------------------------------------------------------------ loaders and unloaders
int AspAudioBufferBatch_DeinterleaveFrom(AspAudioBufferBatch* b, const int16_t* frames, const int32_t* activity, int mem) {
  if (!b) return ASP_ERR_PARAM;
  if (!frames || !good_mem(mem)) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_DeinterleaveFrom: NULL frames or bad mem");
  if (b->P != b->Pin)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_DeinterleaveFrom: the geometry resamples its input (use CopyFrom)");
  if (mem == ASP_MEM_DEVICE && !aligned16(frames))
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_DeinterleaveFrom: device frames are not 16-byte aligned");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  init_for_new_data(b);
  if (activity) b->activity.assign(activity, activity + b->S);
  const size_t bytes = (size_t)b->S * b->P * b->Cin * sizeof(int16_t);
  const int16_t* src = frames;
  if (mem == ASP_MEM_HOST) {
    AB_TRY(b->s_io.reserve(bytes));
    AB_TRY(hipMemcpyAsync(b->s_io.p, frames, bytes, hipMemcpyHostToDevice, b->stream));
    src = (const int16_t*)b->s_io.p;
  }
  // channels_->ibuf() of every processing channel: all of it is overwritten, so its RefreshI moves nothing
  InterleaveArgs a{b->ch_i, nullptr, const_cast<int16_t*>(src), b->S, b->P, b->Cin, b->Cp, 0};
  AB_TRY(launch_deinterleave(a, b->stream));
  b->ch.iv = true;
  b->ch.fv = false;
  if (mem == ASP_MEM_HOST) AB_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAudioBufferBatch_InterleaveTo(AspAudioBufferBatch* b, int16_t* frames, int32_t* activity, int data_changed, int mem) {
  if (!b) return ASP_ERR_PARAM;
  if (!good_mem(mem)) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_InterleaveTo: bad mem");
  if (b->P != b->Pout)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_InterleaveTo: the geometry resamples its output (use CopyTo)");
  if (b->num_channels != b->Cin)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_InterleaveTo: num_channels differs from the frame's channels");
  if (activity) memcpy(activity, b->activity.data(), b->S * sizeof(int32_t));
  if (!data_changed) return ASP_OK;
  if (!frames) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_InterleaveTo: NULL frames");
  if (mem == ASP_MEM_DEVICE && !aligned16(frames))
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_InterleaveTo: device frames are not 16-byte aligned");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  const size_t bytes = (size_t)b->S * b->P * b->Cin * sizeof(int16_t);
  int16_t* dst = frames;
  if (mem == ASP_MEM_HOST) {
    AB_TRY(b->s_io.reserve(bytes));
    dst = (int16_t*)b->s_io.p;
  }
  // channels_->ibuf(): RefreshI when the int16 side is stale (here inside the same launch), the float side stale after
  InterleaveArgs a{b->ch_i, b->ch_f, dst, b->S, b->P, b->Cin, b->Cp, b->ch.iv ? 0 : 1};
  AB_TRY(launch_interleave(a, b->stream));
  b->ch.iv = true;
  b->ch.fv = false;
  if (mem == ASP_MEM_HOST) {
    AB_TRY(hipMemcpyAsync(frames, dst, bytes, hipMemcpyDeviceToHost, b->stream));
    AB_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}

int AspAudioBufferBatch_CopyFrom(AspAudioBufferBatch* b, const float* data, int layout, int mem) {
  if (!b) return ASP_ERR_PARAM;
  if (!data || !good_mem(mem)) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_CopyFrom: NULL data or bad mem");
  if (layout < ASP_AB_MONO || layout > ASP_AB_STEREO_AND_KEYBOARD)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_CopyFrom: bad layout");
  const bool kb = layout >= ASP_AB_MONO_AND_KEYBOARD;
  if ((layout & 1) + 1 != b->Cin)
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_CopyFrom: the layout's channels differ from num_input_channels");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  init_for_new_data(b);
  const int Cio = b->Cin + (kb ? 1 : 0);
  if (kb) b->keyboard = data + (size_t)b->Cin * b->Pin;
  CopyArgs a;
  memset(&a, 0, sizeof a);
  a.src_frames = b->Pin;
  a.dst_frames = b->P;
  a.S = b->S;
  a.Cp = b->Cp;
  a.Cin = b->Cin;
  a.Cio = Cio;
  a.out = b->ch_f;
  if (b->rs_in) {
    if (!plan_push(&b->in_res, &a.plan[0])) return ab_fail(ASP_ERR_STATE, "AspAudioBufferBatch_CopyFrom: resampler plan");
    a.plan[1] = a.plan[0];
    a.state = b->rs_in;
    a.ktable = b->kt_in;
    a.buf_len = b->in_res.buf_len;
    AB_TRY(b->ring_in.upload(b->in_res.desc_host, b->stream, &a.desc));
  }
  const size_t bytes = (size_t)b->S * Cio * b->Pin * sizeof(float);
  a.in_f = data;
  if (mem == ASP_MEM_HOST) {
    AB_TRY(b->s_io.reserve(bytes));
    AB_TRY(hipMemcpyAsync(b->s_io.p, data, bytes, hipMemcpyHostToDevice, b->stream));
    a.in_f = (const float*)b->s_io.p;
  }
  // channels_->fbuf() of every processing channel: overwritten whole; the int16 side is stale after
  AB_TRY(launch_copy(a, true, b->stream));
  if (b->rs_in) AB_TRY(b->ring_in.mark(b->stream));
  b->ch.fv = true;
  b->ch.iv = false;
  if (mem == ASP_MEM_HOST) AB_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAudioBufferBatch_CopyTo(AspAudioBufferBatch* b, float* data, int mem) {
  if (!b) return ASP_ERR_PARAM;
  if (!data || !good_mem(mem)) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_CopyTo: NULL data or bad mem");
  const int nc = b->num_channels;
  if (nc < 1 || nc > b->Cp) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_CopyTo: num_channels outside 1 .. num_proc_channels");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  CopyArgs a;
  memset(&a, 0, sizeof a);
  a.src_frames = b->P;
  a.dst_frames = b->Pout;
  a.S = b->S;
  a.Cp = b->Cp;
  a.Cin = b->Cin;
  a.Cio = nc;
  a.in_f = b->ch_f;
  // channels_->fbuf(): RefreshF of the whole pair when the float side is stale -- inside the launch when the launch
  // covers every processing channel, in front of it otherwise -- and the int16 side stale after
  if (!b->ch.fv) {
    if (nc == b->Cp) {
      a.in_i = b->ch_i;
      a.refresh_f = b->ch_f;
    } else {
      AB_TRY(launch_refresh_f(RefreshFArgs{b->ch_i, b->ch_f, (int)(b->U() * b->P / kGroup)}, b->stream));
    }
  }
  if (b->rs_out) {
    // output_resamplers_[i] for i < num_channels: channels whose resamplers have the same history share a plan
    std::vector<OutDesc> all;
    const SincPos before0 = get_pos(&b->out_res[0]);
    for (int c = 0; c < nc; ++c) {
      if (c > 0 && same_pos(get_pos(&b->out_res[c]), before0)) {
        set_pos(&b->out_res[c], get_pos(&b->out_res[0]));
        a.plan[c] = a.plan[0];
        a.desc_off[c] = 0;
        continue;
      }
      if (!plan_push(&b->out_res[c], &a.plan[c])) return ab_fail(ASP_ERR_STATE, "AspAudioBufferBatch_CopyTo: resampler plan");
      a.desc_off[c] = (int)all.size();
      all.insert(all.end(), b->out_res[c].desc_host.begin(), b->out_res[c].desc_host.end());
    }
    a.state = b->rs_out;
    a.ktable = b->kt_out;
    a.buf_len = b->out_res[0].buf_len;
    AB_TRY(b->ring_out.upload(all, b->stream, &a.desc));
  }
  const size_t bytes = (size_t)b->S * nc * b->Pout * sizeof(float);
  a.out = data;
  if (mem == ASP_MEM_HOST) {
    AB_TRY(b->s_io.reserve(bytes));
    a.out = (float*)b->s_io.p;
  }
  AB_TRY(launch_copy(a, false, b->stream));
  if (b->rs_out) AB_TRY(b->ring_out.mark(b->stream));
  b->ch.fv = true;
  b->ch.iv = false;
  if (mem == ASP_MEM_HOST) {
    AB_TRY(hipMemcpyAsync(data, a.out, bytes, hipMemcpyDeviceToHost, b->stream));
    AB_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}

// ------------------------------------------------------------------ bands
int AspAudioBufferBatch_SplitIntoFrequencyBands(AspAudioBufferBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  if (!b->has_bands) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_SplitIntoFrequencyBands: the buffer has no bands");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  // SplittingFilter::Analysis: in_data->ibuf_const(), every band's ibuf() (written whole)
  if (int rc = touch(b, -1, false, true)) return rc;
  if (int rc = AspSplitBatch_Analysis(b->split, b->ch_i, b->band_i, ASP_MEM_DEVICE)) return rc;
  for (int k = 0; k < b->nb; ++k) {
    b->band[k].iv = true;
    b->band[k].fv = false;
  }
  return ASP_OK;
}

int AspAudioBufferBatch_MergeFrequencyBands(AspAudioBufferBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  if (!b->has_bands) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_MergeFrequencyBands: the buffer has no bands");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  // SplittingFilter::Synthesis: every band's ibuf_const(), out_data->ibuf() (written whole)
  if (int rc = refresh_set(b, nullptr, nullptr)) return rc;
  if (int rc = AspSplitBatch_Synthesis(b->split, b->band_i, b->ch_i, ASP_MEM_DEVICE)) return rc;
  b->ch.iv = true;
  b->ch.fv = false;
  return ASP_OK;
}

int AspAudioBufferBatch_CopyLowPassToReference(AspAudioBufferBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  b->ref_copied = true;
  return refresh_set(b, nullptr, b->ref);  // split_bands_const(i)[kBand0To8kHz] of every channel
}

const int16_t* AspAudioBufferBatch_low_pass_reference(AspAudioBufferBatch* b) { return b && b->ref_copied ? b->ref : nullptr; }

const int16_t* AspAudioBufferBatch_mixed_low_pass_data(AspAudioBufferBatch* b) {
  if (!b) return nullptr;
  AspDeviceScope dev_scope_;
  if (dev_scope_.select(b->device) != hipSuccess) return nullptr;
  if (b->Cp == 1)  // split_bands_const(0)[kBand0To8kHz]
    return refresh_set(b, nullptr, nullptr) == ASP_OK ? bands_of(b).bi : nullptr;
  if (!b->mixed_valid) {
    if (refresh_set(b, b->mixed, nullptr) != ASP_OK) return nullptr;
    b->mixed_valid = true;
  }
  return b->mixed;
}

// ------------------------------------------------------------------ views
int16_t* AspAudioBufferBatch_channels(AspAudioBufferBatch* b) { return (int16_t*)view(b, -1, false, false, "AspAudioBufferBatch_channels"); }
const int16_t* AspAudioBufferBatch_channels_const(AspAudioBufferBatch* b) {
  return (const int16_t*)view(b, -1, false, true, "AspAudioBufferBatch_channels_const");
}
float* AspAudioBufferBatch_channels_f(AspAudioBufferBatch* b) { return (float*)view(b, -1, true, false, "AspAudioBufferBatch_channels_f"); }
const float* AspAudioBufferBatch_channels_const_f(AspAudioBufferBatch* b) {
  return (const float*)view(b, -1, true, true, "AspAudioBufferBatch_channels_const_f");
}
int16_t* AspAudioBufferBatch_split_channels(AspAudioBufferBatch* b, int band) {
  return band < 0 ? nullptr : (int16_t*)view(b, band, false, false, "AspAudioBufferBatch_split_channels");
}
const int16_t* AspAudioBufferBatch_split_channels_const(AspAudioBufferBatch* b, int band) {
  return band < 0 ? nullptr : (const int16_t*)view(b, band, false, true, "AspAudioBufferBatch_split_channels_const");
}
float* AspAudioBufferBatch_split_channels_f(AspAudioBufferBatch* b, int band) {
  return band < 0 ? nullptr : (float*)view(b, band, true, false, "AspAudioBufferBatch_split_channels_f");
}
const float* AspAudioBufferBatch_split_channels_const_f(AspAudioBufferBatch* b, int band) {
  return band < 0 ? nullptr : (const float*)view(b, band, true, true, "AspAudioBufferBatch_split_channels_const_f");
}

// ------------------------------------------------------------------ scalars
int AspAudioBufferBatch_num_channels(const AspAudioBufferBatch* b) { return b ? b->num_channels : ASP_ERR_PARAM; }
int AspAudioBufferBatch_set_num_channels(AspAudioBufferBatch* b, int num_channels) {
  if (!b) return ASP_ERR_PARAM;
  b->num_channels = num_channels;
  return ASP_OK;
}
int AspAudioBufferBatch_num_bands(const AspAudioBufferBatch* b) { return b ? b->nb : ASP_ERR_PARAM; }
int AspAudioBufferBatch_samples_per_channel(const AspAudioBufferBatch* b) { return b ? b->P : ASP_ERR_PARAM; }
int AspAudioBufferBatch_samples_per_split_channel(const AspAudioBufferBatch* b) { return b ? b->ns : ASP_ERR_PARAM; }
int AspAudioBufferBatch_samples_per_keyboard_channel(const AspAudioBufferBatch* b) { return b ? b->Pin : ASP_ERR_PARAM; }
const float* AspAudioBufferBatch_keyboard_data(const AspAudioBufferBatch* b) { return b ? b->keyboard : nullptr; }
int AspAudioBufferBatch_set_activity(AspAudioBufferBatch* b, int stream, int activity) {
  if (!b || stream < 0 || stream >= b->S) return ASP_ERR_PARAM;
  b->activity[stream] = activity;
  return ASP_OK;
}
int AspAudioBufferBatch_activity(const AspAudioBufferBatch* b, int stream) {
  return b && stream >= 0 && stream < b->S ? b->activity[stream] : ASP_ERR_PARAM;
}

// ------------------------------------------------------------------ plumbing
int AspAudioBufferBatch_Read(AspAudioBufferBatch* b, int what, int band, void* host_dst, int* valid) {
  if (!b || !host_dst) return ASP_ERR_PARAM;
  const void* src = nullptr;
  size_t bytes = 0;
  int ok = 0;
  if (what == ASP_AB_READ_I16 || what == ASP_AB_READ_F32) {
    const bool f = what == ASP_AB_READ_F32;
    if (band >= 0 && (!b->has_bands || band >= b->nb)) return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Read: no such band");
    const Pair& p = band < 0 ? b->ch : b->band[band];
    const size_t len = b->U() * (band < 0 ? b->P : kBandSamples), off = band < 0 ? 0 : band * len;
    src = f ? (const void*)((band < 0 ? b->ch_f : b->band_f) + off) : (const void*)((band < 0 ? b->ch_i : b->band_i) + off);
    bytes = len * (f ? sizeof(float) : sizeof(int16_t));
    ok = f ? p.fv : p.iv;
  } else if (what == ASP_AB_READ_MIXED) {
    src = b->mixed;
    bytes = (size_t)b->S * b->ns * sizeof(int16_t);
    ok = b->mixed_valid;
  } else if (what == ASP_AB_READ_REFERENCE) {
    src = b->ref;
    bytes = b->U() * b->ns * sizeof(int16_t);
    ok = b->ref_copied;
  } else {
    return ab_fail(ASP_ERR_PARAM, "AspAudioBufferBatch_Read: bad selector");
  }
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  AB_TRY(hipMemcpyAsync(host_dst, src, bytes, hipMemcpyDeviceToHost, b->stream));
  AB_TRY(hipStreamSynchronize(b->stream));
  if (valid) *valid = ok;
  return ASP_OK;
}

int AspAudioBufferBatch_kernel_table(const AspAudioBufferBatch* b, int which, float* out, int capacity) {
  if (!b || !out || (which != 0 && which != 1)) return 0;
  const SincHost& r = which == 0 ? b->in_res : b->out_res[0];
  if ((which == 0 ? b->rs_in : b->rs_out) == nullptr || capacity < (int)r.kernel_host.size()) return 0;
  memcpy(out, r.kernel_host.data(), r.kernel_host.size() * sizeof(float));
  return (int)r.kernel_host.size();
}

int AspAudioBufferBatch_SetStream(AspAudioBufferBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  AB_TRY(hipStreamSynchronize(b->stream));
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return b->split ? AspSplitBatch_SetStream(b->split, b->stream) : ASP_OK;
}

int AspAudioBufferBatch_Synchronize(AspAudioBufferBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  AB_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

size_t AspAudioBufferBatch_state_size(const AspAudioBufferBatch* b) {
  if (!b) return 0;
  size_t per = 0;
  if (b->rs_in) per += b->in_res.buf_len * sizeof(float);
  if (b->rs_out) per += b->out_res[0].buf_len * sizeof(float);
  if (b->split) per += sizeof(AspSplitState);
  return sizeof(AbRecord) + per * b->Cp;
}

int AspAudioBufferBatch_ExportState(AspAudioBufferBatch* b, int stream, void* blob) {
  if (!b || !blob || stream < 0 || stream >= b->S) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  char* p = (char*)blob;
  const AbRecord r = record_of(b);
  memcpy(p, &r, sizeof r);
  p += sizeof r;
  for (int c = 0; c < b->Cp; ++c) {
    const size_t u = (size_t)stream * b->Cp + c;
    if (b->rs_in) {
      const size_t n = b->in_res.buf_len * sizeof(float);
      AB_TRY(hipMemcpyAsync(p, b->rs_in + u * b->in_res.buf_len, n, hipMemcpyDeviceToHost, b->stream));
      p += n;
    }
    if (b->rs_out) {
      const size_t n = b->out_res[0].buf_len * sizeof(float);
      AB_TRY(hipMemcpyAsync(p, b->rs_out + u * b->out_res[0].buf_len, n, hipMemcpyDeviceToHost, b->stream));
      p += n;
    }
    if (b->split) {
      AspSplitState st;
      if (int rc = AspSplitBatch_ExportState(b->split, (int)u, &st)) return rc;
      memcpy(p, &st, sizeof st);
      p += sizeof st;
    }
  }
  AB_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAudioBufferBatch_ImportState(AspAudioBufferBatch* b, int stream, const void* blob) {
  if (!b || !blob || stream < 0 || stream >= b->S) return ASP_ERR_PARAM;
  const char* p = (const char*)blob;
  AbRecord r;
  memcpy(&r, p, sizeof r);
  p += sizeof r;
  const AbRecord mine = record_of(b);
  bool same = r.magic == kRecordMagic && memcmp(r.geometry, mine.geometry, sizeof r.geometry) == 0 &&
              same_pos(r.in_pos, mine.in_pos);
  for (int c = 0; c < 2; ++c) same = same && same_pos(r.out_pos[c], mine.out_pos[c]);
  if (!same)
    return ab_fail(ASP_ERR_STATE, "AspAudioBufferBatch_ImportState: the blob's geometry or position record differs from the batch's");
  AspDeviceScope dev_scope_;
  AB_TRY(dev_scope_.select(b->device));
  for (int c = 0; c < b->Cp; ++c) {
    const size_t u = (size_t)stream * b->Cp + c;
    const char* q = p;
    if (b->rs_in) q += b->in_res.buf_len * sizeof(float);
    if (b->rs_out) q += b->out_res[0].buf_len * sizeof(float);
    if (b->split) {  // first: the band split is what can still refuse
      AspSplitState st;
      memcpy(&st, q, sizeof st);
      if (int rc = AspSplitBatch_ImportState(b->split, (int)u, &st)) return rc;
      q += sizeof st;
    }
    if (b->rs_in) {
      const size_t n = b->in_res.buf_len * sizeof(float);
      AB_TRY(hipMemcpyAsync(b->rs_in + u * b->in_res.buf_len, p, n, hipMemcpyHostToDevice, b->stream));
      p += n;
    }
    if (b->rs_out) {
      const size_t n = b->out_res[0].buf_len * sizeof(float);
      AB_TRY(hipMemcpyAsync(b->rs_out + u * b->out_res[0].buf_len, p, n, hipMemcpyHostToDevice, b->stream));
      p += n;
    }
    p = q;
  }
  AB_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

}  // extern "C"
