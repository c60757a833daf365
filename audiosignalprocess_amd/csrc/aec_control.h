// aec_control.h -- the echo canceller's host control plane: the reference's integer bookkeeping per call
// (echo_cancellation.c:196-409,594-742,816-922; aec_core.c:1618-1778; ring positions of
// common_audio/ring_buffer.c; EstimateSkew of aec_resampler.c) on plain data.  A call updates one stream's AecCtl
// (and, where the state is the batch's, the AecSetup) and hands the device work it asks for -- launch descriptors of
// aec_layout.h -- to an AecIssuer.  Host-only: no HIP header, nothing here touches a device.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "aec_layout.h"
#include "asp_aec.h"

#pragma GCC visibility push(hidden)  // one copy per program that includes it, none of it exported
namespace aspaec {

// ------------------------------------------------------------ ring positions
struct RingPos {  // common_audio/ring_buffer.c:26-33 without the data
  int read, write, wrap, count;
};
inline void rp_init(RingPos* r, int count) {
  r->read = 0;
  r->write = 0;
  r->wrap = 0;
  r->count = count;
}
inline int rp_avail_read(const RingPos* r) {
  return r->wrap == 0 ? r->write - r->read : r->count - r->read + r->write;
}
inline int rp_avail_write(const RingPos* r) { return r->count - rp_avail_read(r); }
inline int rp_move_read(RingPos* r, int n) {  // WebRtc_MoveReadPtr, ring_buffer.c:195-228
  const int free_elements = rp_avail_write(r), readable = rp_avail_read(r);
  int pos = r->read;
  if (n > readable) n = readable;
  if (n < -free_elements) n = -free_elements;
  pos += n;
  if (pos > r->count) {
    pos -= r->count;
    r->wrap = 0;
  }
  if (pos < 0) {
    pos += r->count;
    r->wrap = 1;
  }
  r->read = pos;
  return n;
}
// WebRtc_WriteBuffer positions (ring_buffer.c:161-192): returns the elements written; *start is
// the position the first element lands on (the device adds i modulo count).
inline int rp_write(RingPos* r, int n, int* start) {
  const int free_elements = rp_avail_write(r);
  const int write_elements = free_elements < n ? free_elements : n;
  int m = write_elements;
  const int margin = r->count - r->write;
  *start = r->write;
  if (write_elements > margin) {
    r->write = 0;
    m -= margin;
    r->wrap = 1;
  }
  r->write += m;
  return write_elements;
}
// WebRtc_ReadBuffer positions (ring_buffer.c:112-158)
inline int rp_read(RingPos* r, int n, int* start) {
  const int readable = rp_avail_read(r);
  const int read_elements = readable < n ? readable : n;
  *start = r->read;
  rp_move_read(r, read_elements);
  return read_elements;
}

constexpr int kInitCheck = 42;           // echo_cancellation.c:59
constexpr int kMaxTrustedDelayMs = 500;  // :53
constexpr int kMaxBufSizeStart = 62;     // :57
constexpr int kSampMsNb = 8;             // :58

// EstimateSkew (aec_resampler.c:143-217): least-squares slope of the cumulated, outlier-cleaned skew reports
inline int estimate_skew(const int* rawSkew, int size, int deviceSampleRateHz, float* skewEst) {
  const int absLimitOuter = (int)(0.04f * deviceSampleRateHz);
  const int absLimitInner = (int)(0.0025f * deviceSampleRateHz);
  int n = 0;
  float rawAvg = 0, err = 0, rawAbsDev = 0, cumSum = 0, x = 0, x2 = 0, y = 0, xy = 0, xAvg = 0, denom = 0, skew = 0;
  *skewEst = 0;
  for (int i = 0; i < size; i++) {
    if ((rawSkew[i] < absLimitOuter && rawSkew[i] > -absLimitOuter)) {
      n++;
      rawAvg += rawSkew[i];
    }
  }
  if (n == 0) return -1;
  rawAvg /= n;
  for (int i = 0; i < size; i++) {
    if ((rawSkew[i] < absLimitOuter && rawSkew[i] > -absLimitOuter)) {
      err = rawSkew[i] - rawAvg;
      rawAbsDev += err >= 0 ? err : -err;
    }
  }
  rawAbsDev /= n;
  const int upperLimit = (int)(rawAvg + 5 * rawAbsDev + 1);
  const int lowerLimit = (int)(rawAvg - 5 * rawAbsDev - 1);
  n = 0;
  for (int i = 0; i < size; i++) {
    if ((rawSkew[i] < absLimitInner && rawSkew[i] > -absLimitInner) ||
        (rawSkew[i] < upperLimit && rawSkew[i] > lowerLimit)) {
      n++;
      cumSum += rawSkew[i];
      x += n;
      x2 += n * n;
      y += cumSum;
      xy += n * cumSum;
    }
  }
  if (n == 0) return -1;
  xAvg = x / n;
  denom = x2 - xAvg * x;
  if (denom != 0) skew = (xy - xAvg * y) / denom;
  *skewEst = skew;
  return 0;
}

// ------------------------------------------------------------ state
// What is one for the whole batch, also when every stream has its own control plane: rates, modes, and the parts
// of the control plane that exist only while the batch is fed in lock-step.
struct AecSetup {
  // Aec (echo_cancellation_internal.h:17-65) and the integer part of AecCore (aec_core_internal.h:52-164)
  int sampFreq = 0, scSampFreq = 0, splitSampFreq = 0, rate_factor = 0, initFlag = 0;
  float sampFactor = 1.f;
  int mult = 0;
  int num_high = 0;  // 32 kHz: one high band (aec_core.c:1032-1067)
  float normal_mu = 0.f, normal_error_threshold = 0.f;
  // WebRtcAec_enable_delay_correction (aec_core.c:1876-1881): the extended filter, 32 partitions instead of 12
  int extended = 0, num_part = kNumPartNormal;
  int nlp_mode = 1, skewMode = 0, metricsMode = 0, delay_logging = 0, reported_delay_enabled = 1;
  // skew compensation (set_config skewMode; echo_cancellation.c:304-313, 614-645, aec_resampler.c): the skew estimate
  // and the resampler's position are functions of the calls' skew arguments alone -- one copy for the batch, on the
  // host; the resampler's sample buffer is per stream, on the device
  int skewFrCtr = 0, resample = 0;
  float skew = 0.f, rs_position = 0.f, rs_skewEstimate = 0.f;
  int rs_skewDataIndex = 0, rs_skewData[kSkewEstimateFrames] = {};
  // delay-agnostic mode: once it has taken over the streams' far-buffer read sides (agn_synced), the BufferFarend
  // calls the device has yet to replay
  bool agn_synced = false;
  int nevents = 0, ev_samples[kMaxFarEvents] = {}, ev_parts[kMaxFarEvents] = {};
  // a BufferFarend whose device work is deferred into the next Process launch (Run / TimedSteps)
  bool far_pending = false;
  FarOps far_ops{};
  const float* far_src = nullptr;
};

// The control plane of ONE stream: what two streams of a batch can hold different values of once a caller drives
// them apart (per-stream reported delays, a stream re-initialised: AspAecBatch_ProcessV / _InitStream).  A batch fed
// in lock-step has one of these, otherwise one per stream.
struct AecCtl {
  int lastError = 0, farend_started = 0;
  int bufSizeStart = 0, knownDelay = 0, timeForDelayChange = 0, startup_phase = 0, checkBuffSize = 0, sum = 0;
  int16_t counter = 0, firstVal = 0, checkBufSizeCtr = 0, msInSndCardBuf = 0, filtDelay = 0, lastDelayDiff = 0;
  int system_delay = 0, core_knownDelay = 0;
  int xf_pos = 0, xfw_head = 0, blocks_processed = 0;
  RingPos pre_pos{}, far_pos{}, near_pos{}, out_pos{};
};

// ------------------------------------------------------------ the issue seam
// Everything a control step wants from the device.  Each returns 0 or the error to hand back to the caller.
struct AecIssuer {
  // the delay-agnostic mode goes out as one process descriptor per call (with AgnOps) instead of a delay and a
  // process descriptor per sub-frame
  bool agn_fused = false;
  virtual int farend(const float* far, const FarOps& ops) = 0;
  // sub >= 0: the descriptor covers sub-frame `sub` of the call alone (the unfused delay-agnostic mode)
  virtual int process(int n, const ProcOps& ops, const float* far_src, const FarOps& fops, const AgnOps* agn = nullptr,
                      int sub = -1) = 0;
  virtual int pass_through(int n) = 0;  // the near end of this call goes out unchanged
  virtual int delay(const DelayOps& d) = 0;
  virtual int resample(const float** far, int n, int n_out, float be, float position) = 0;  // *far: the resampled frame

 protected:
  ~AecIssuer() = default;
};

// records the text in the embedding program's error record, returns ASP_ERR_STATE
int aec_refuse(const char* what);

// ------------------------------------------------------------ control functions
// The control plane as WebRtcAec_Init leaves it (echo_cancellation.c:196-276; WebRtcAec_InitAec, aec_core.c:1460-1615):
// one stream's share ...
inline void init_stream_control(AecCtl& c) {
  rp_init(&c.near_pos, kFrBufLen);
  rp_init(&c.out_pos, kFrBufLen);
  rp_init(&c.far_pos, kFarSlots);
  c.system_delay = 0;
  c.core_knownDelay = 0;
  c.xf_pos = 0;
  c.xfw_head = 0;
  c.blocks_processed = 0;
  rp_init(&c.pre_pos, kPreLen);
  rp_move_read(&c.pre_pos, -kPartLen);  // start overlap, echo_cancellation.c:226
  c.sum = 0;
  c.counter = 0;
  c.checkBuffSize = 1;
  c.firstVal = 0;
  c.startup_phase = 1;  // = reported_delay_enabled, which InitAec has just set (echo_cancellation.c:247)
  c.bufSizeStart = 0;
  c.checkBufSizeCtr = 0;
  c.msInSndCardBuf = 0;
  c.filtDelay = -1;
  c.timeForDelayChange = 0;
  c.knownDelay = 0;
  c.lastDelayDiff = 0;
  c.farend_started = 0;
}
// ... and the batch's with it, the default configuration (:261-270) included
inline void init_control(AecSetup& su, AecCtl& c, int32_t sampFreq, int32_t scSampFreq) {
  su.sampFreq = sampFreq;
  su.scSampFreq = scSampFreq;
  if (sampFreq == 8000) {
    su.normal_mu = 0.6f;
    su.normal_error_threshold = 2e-6f;
  } else {
    su.normal_mu = 0.5f;
    su.normal_error_threshold = 1.5e-6f;
  }
  su.num_high = sampFreq == 32000 ? 1 : 0;           // aec_core.c:1466-1473
  su.mult = sampFreq == 32000 ? 2 : sampFreq / 8000;  // aec_core.c:1541-1545
  su.extended = 0;                                    // aec_core.c:1522-1523
  su.num_part = kNumPartNormal;
  su.rs_position = 0.f;
  su.rs_skewDataIndex = 0;
  su.rs_skewEstimate = 0.f;
  memset(su.rs_skewData, 0, sizeof su.rs_skewData);
  su.skewFrCtr = 0;  // echo_cancellation.c:256-259
  su.resample = kAecFalse;
  su.skew = 0.f;
  su.reported_delay_enabled = 1;  // aec_core.c:1517-1521 (not Android)
  su.agn_synced = false;
  su.nevents = 0;
  su.initFlag = kInitCheck;
  su.splitSampFreq = sampFreq == 32000 ? 16000 : sampFreq;  // echo_cancellation.c:231-235
  su.rate_factor = su.splitSampFreq / 8000;
  su.sampFactor = (su.scSampFreq * 1.0f) / su.splitSampFreq;  // echo_cancellation.c:237
  su.far_pending = false;
  su.nlp_mode = kAecNlpModerate;
  su.skewMode = kAecFalse;
  su.metricsMode = kAecFalse;
  su.delay_logging = kAecFalse;
  init_stream_control(c);
}

inline int far_move_read(AecCtl& c, int elements) {  // WebRtcAec_MoveFarReadPtr, aec_core.c:1637-1645
  const int moved = rp_move_read(&c.far_pos, elements);
  c.system_delay -= moved * kPartLen;
  return moved;
}

inline int flush_pending_farend(AecSetup& su, AecIssuer& iss) {
  if (!su.far_pending) return 0;
  su.far_pending = false;
  return iss.farend(su.far_src, su.far_ops);
}

// Delay-agnostic mode with more far-end calls waiting than a descriptor holds: replay them now (no sub-frame follows).
inline int flush_far_events(AecSetup& su, AecIssuer& iss) {
  DelayOps d;
  memset(&d, 0, sizeof d);
  d.control = 2;
  d.mult = su.mult;
  d.num_part = su.num_part;
  d.nevents = su.nevents;
  memcpy(d.ev_samples, su.ev_samples, sizeof d.ev_samples);
  memcpy(d.ev_parts, su.ev_parts, sizeof d.ev_parts);
  su.nevents = 0;
  return iss.delay(d);
}

// WebRtcAec_BufferFarend control plane (echo_cancellation.c:278-339).
// defer = true: when the call needs one launch descriptor (the normal case) its device work is
// kept for the following Process launch instead of being issued on its own.
inline int buffer_farend_device(AecSetup& su, AecCtl& c, AecIssuer& iss, const float* far, int n, bool defer = false) {
  if (const int rc = flush_pending_farend(su, iss)) return rc;
  if (su.skewMode == kAecTrue && su.resample == kAecTrue) {
    // WebRtcAec_ResampleLinear (aec_resampler.c:74-123): the sample positions follow from the skew and the
    // resampler's position alone, so the output length and the new position are computed here, once; the device
    // interpolates every stream's samples with the same float expressions
    const float be = 1 + su.skew;
    int mm = 0;
    float tnew = be * mm + su.rs_position;
    int tn = (int)tnew;
    while (tn < n) {
      mm++;
      tnew = be * mm + su.rs_position;
      tn = (int)tnew;
    }
    if (const int rc = iss.resample(&far, n, mm, be, su.rs_position)) return rc;
    su.rs_position += mm * be - n;
    n = mm;
  }
  c.farend_started = 1;
  c.system_delay += n;
  FarOps ops;
  memset(&ops, 0, sizeof ops);
  ops.n = rp_write(&c.pre_pos, n, &ops.wpos);
  bool pending = true;
  int parts_of_call = 0;
  while (rp_avail_read(&c.pre_pos) >= kPartLen2) {
    int rpos;
    rp_read(&c.pre_pos, kPartLen2, &rpos);
    int slot;
    if (su.agn_synced) {
      // the read side (and with it "is the buffer full", aec_core.c:1622-1625) is the stream's own and lives on
      // the device; the write position stays common to the batch: every stream writes one partition here
      slot = c.far_pos.write >= kFarSlots ? c.far_pos.write - kFarSlots : c.far_pos.write;
      c.far_pos.write = slot + 1;
    } else {
      if (rp_avail_write(&c.far_pos) < 1) far_move_read(c, 1);  // aec_core.c:1622-1625
      rp_write(&c.far_pos, 1, &slot);
      if (slot >= kFarSlots) slot -= kFarSlots;
    }
    ++parts_of_call;
    if (ops.nparts == 3) {  // a fourth partition in one call: the full descriptor goes out on its own
      if (const int rc = iss.farend(far, ops)) return rc;
      memset(&ops, 0, sizeof ops);
      pending = false;
    }
    ops.rpos[ops.nparts] = rpos;
    ops.slot[ops.nparts] = slot;
    ops.nparts++;
    rp_move_read(&c.pre_pos, -kPartLen);  // overlap, echo_cancellation.c:336
  }
  if (su.agn_synced) {  // the device replays this call on every stream's own read side at its next control step
    if (su.nevents == kMaxFarEvents) {
      if (const int rc = flush_far_events(su, iss)) return rc;
    }
    su.ev_samples[su.nevents] = n;
    su.ev_parts[su.nevents] = parts_of_call;
    su.nevents++;
  }
  if (pending || ops.nparts > 0) {
    if (defer && pending) {  // everything of this call fits one descriptor
      su.far_pending = true;
      su.far_ops = ops;
      su.far_src = far;
    } else {
      return iss.farend(far, ops);
    }
  }
  return 0;
}

inline void est_buf_delay_normal(const AecSetup& su, AecCtl& c) {  // echo_cancellation.c:816-867
  const int nSampSndCard = c.msInSndCardBuf * kSampMsNb * su.rate_factor;
  int current_delay = nSampSndCard - c.system_delay;
  current_delay += kFrameLen * su.rate_factor;
  if (su.skewMode == kAecTrue && su.resample == kAecTrue) current_delay -= kResamplingDelay;  // echo_cancellation.c:831-833
  if (current_delay < kPartLen) current_delay += far_move_read(c, 1) * kPartLen;
  c.filtDelay = c.filtDelay < 0 ? 0 : c.filtDelay;
  {
    const int16_t v = (int16_t)(0.8 * c.filtDelay + 0.2 * current_delay);
    c.filtDelay = v > 0 ? v : 0;
  }
  const int delay_difference = c.filtDelay - c.knownDelay;
  if (delay_difference > 224) {
    if (c.lastDelayDiff < 96) {
      c.timeForDelayChange = 0;
    } else {
      c.timeForDelayChange++;
    }
  } else if (delay_difference < 96 && c.knownDelay > 0) {
    if (c.lastDelayDiff > 224) {
      c.timeForDelayChange = 0;
    } else {
      c.timeForDelayChange++;
    }
  } else {
    c.timeForDelayChange = 0;
  }
  c.lastDelayDiff = (int16_t)delay_difference;
  if (c.timeForDelayChange > 25) {
    const int v = (int)c.filtDelay - 160;
    c.knownDelay = v > 0 ? v : 0;
  }
}

// The delay-agnostic control step of sub-frame j (aec_core.c:1703-1718, 2 b, runs per stream on the device): the
// first one after Init starts every stream from the batch's values at the call's entry, later ones replay the
// BufferFarend calls since the last.
inline void fill_agn_delay(AecSetup& su, DelayOps& d, int j, int nblocks, const RingPos& far_at_entry, int system_delay_at_entry) {
  memset(&d, 0, sizeof d);
  d.control = 1;
  d.mult = su.mult;
  d.num_part = su.num_part;
  d.nblocks = nblocks;
  if (!su.agn_synced) {
    d.sync = 1;
    d.h_far_read = far_at_entry.read;
    d.h_far_write = far_at_entry.write;
    d.h_far_wrap = far_at_entry.wrap;
    d.h_system_delay = system_delay_at_entry;
    su.agn_synced = true;
    su.nevents = 0;
  } else if (j == 0) {
    d.nevents = su.nevents;
    memcpy(d.ev_samples, su.ev_samples, sizeof d.ev_samples);
    memcpy(d.ev_parts, su.ev_parts, sizeof d.ev_parts);
    su.nevents = 0;
  }
}

// What every Process descriptor of a batch has alike: the fields that follow from the setup alone.
inline ProcOps batch_proc_ops(const AecSetup& su) {
  ProcOps ops;
  memset(&ops, 0, sizeof ops);
  ops.mult = su.mult;
  ops.nlp_mode = su.nlp_mode;
  ops.num_high = su.num_high;
  ops.mu = su.extended ? 0.4f : su.normal_mu;                                 // kExtendedMu, aec_core.c:172
  ops.error_threshold = su.extended ? 1.0e-6f : su.normal_error_threshold;    // kExtendedErrorThreshold, :173-175
  return ops;
}

// WebRtcAec_ProcessFrames control plane (aec_core.c:1647-1778) -> one process descriptor.
// `knownDelay`: the delay ProcessNormal / ProcessExtended hand over (echo_cancellation.c:735-741, 803-812)
inline int process_frames_device(AecSetup& su, AecCtl& c, AecIssuer& iss, int n, int knownDelay) {
  ProcOps ops = batch_proc_ops(su);
  const RingPos far_at_entry = c.far_pos;  // what the agnostic mode's first control step starts every stream from
  const int system_delay_at_entry = c.system_delay;
  const int kNumPart = su.num_part;
  for (int j = 0; j < n; j += kFrameLen) {
    SubFrame& sf = ops.sub[ops.nsub++];
    rp_write(&c.near_pos, kFrameLen, &sf.near_wpos);
    if (c.system_delay < kFrameLen) far_move_read(c, -(su.mult + 1));
    if (su.reported_delay_enabled) {  // 2 a) aec_core.c:1703-1718
      const int move_elements = (c.core_knownDelay - knownDelay - 32) / kPartLen;
      const int moved_elements = rp_move_read(&c.far_pos, move_elements);
      c.core_knownDelay -= moved_elements * kPartLen;
    }
    while (rp_avail_read(&c.near_pos) >= kPartLen) {
      if (sf.nblocks >= 2) return aec_refuse("more than two blocks in one sub-frame");
      BlockOp& op = sf.blk[sf.nblocks++];
      rp_read(&c.near_pos, kPartLen, &op.near_rpos);
      int slot;
      rp_read(&c.far_pos, 1, &slot);
      op.far_slot = slot >= kFarSlots ? slot - kFarSlots : slot;
      c.xf_pos = c.xf_pos == 0 ? kNumPart - 1 : c.xf_pos - 1;  // aec_core.c:1203-1207
      c.xfw_head = (c.xfw_head + kNumPartMax - 1) % kNumPartMax;
      op.xf_pos = c.xf_pos;
      op.xfw_head = c.xfw_head;
      rp_write(&c.out_pos, kPartLen, &op.out_wpos);
      c.blocks_processed++;
    }
    c.system_delay -= kFrameLen;
    const int out_elements = rp_avail_read(&c.out_pos);
    if (out_elements < kFrameLen) rp_move_read(&c.out_pos, out_elements - kFrameLen);
    rp_read(&c.out_pos, kFrameLen, &sf.out_rpos);
  }
  const float* far_src = nullptr;
  FarOps fops;
  memset(&fops, 0, sizeof fops);
  if (su.far_pending) {
    su.far_pending = false;
    far_src = su.far_src;
    fops = su.far_ops;
  }
  ops.spectra = su.delay_logging;
  DelayOps d;
  if (su.reported_delay_enabled) {
    if (const int rc = iss.process(n, ops, far_src, fops)) return rc;
    if (!su.delay_logging) return 0;
    memset(&d, 0, sizeof d);  // the estimator takes the blocks of this call (aec_core.c:1191-1203)
    for (int j = 0; j < ops.nsub; ++j) d.npending += ops.sub[j].nblocks;
    d.logging = 1;
    d.mult = su.mult;
    d.num_part = su.num_part;
    return d.npending > 0 ? iss.delay(d) : 0;
  }
  // ---- delay-agnostic mode: per 80-sample sub-frame the per-stream control step (with the estimator's share of the
  // previous sub-frame's blocks), then the blocks themselves with the far slots that step chose
  // (An issuer without a device refuses these descriptors only after fill_agn_delay has marked the batch synced.  No
  // state is lost by that: such a handle never gets here, enable_reported_delay(0) is refused on it.)
  ops.agnostic = 1;
  if (iss.agn_fused) {
    // one descriptor per call: every stream's wave runs its own control steps and the estimator between its blocks
    // (aec_kernels.hip, process_call<AGN>)
    AgnOps agn;
    memset(&agn, 0, sizeof agn);
    agn.logging = su.delay_logging;
    for (int j = 0; j < ops.nsub; ++j) fill_agn_delay(su, agn.sub[j], j, ops.sub[j].nblocks, far_at_entry, system_delay_at_entry);
    return iss.process(n, ops, far_src, fops, &agn);
  }
  int prev_blocks = 0;
  for (int j = 0; j < ops.nsub; ++j) {
    fill_agn_delay(su, d, j, ops.sub[j].nblocks, far_at_entry, system_delay_at_entry);
    d.npending = su.delay_logging ? prev_blocks : 0;
    d.logging = su.delay_logging;
    if (const int rc = iss.delay(d)) return rc;
    ProcOps one = ops;
    one.nsub = 1;
    one.sub[0] = ops.sub[j];
    if (const int rc = iss.process(n, one, j == 0 ? far_src : nullptr, fops, nullptr, j)) return rc;
    prev_blocks = ops.sub[j].nblocks;
  }
  if (su.delay_logging && prev_blocks > 0) {  // the last sub-frame's blocks
    memset(&d, 0, sizeof d);
    d.npending = prev_blocks;
    d.logging = 1;
    d.mult = su.mult;
    d.num_part = su.num_part;
    return iss.delay(d);
  }
  return 0;
}

// ProcessNormal (echo_cancellation.c:594-742).
inline int process_normal_device(AecSetup& su, AecCtl& c, AecIssuer& iss, int n, int16_t msInSndCardBuf, int32_t skew,
                                 int* rc_ref) {
  const int nBlocks10ms = n / (kFrameLen * su.rate_factor);
  msInSndCardBuf = msInSndCardBuf > kMaxTrustedDelayMs ? kMaxTrustedDelayMs : msInSndCardBuf;
  msInSndCardBuf += 10;
  c.msInSndCardBuf = msInSndCardBuf;
  if (su.skewMode == kAecTrue) {  // echo_cancellation.c:614-645
    if (su.skewFrCtr < 25) {
      su.skewFrCtr++;
    } else {
      int err = 0;  // WebRtcAec_GetSkew, aec_resampler.c:125-141
      if (su.rs_skewDataIndex < kSkewEstimateFrames) {
        su.rs_skewData[su.rs_skewDataIndex] = skew;
        su.rs_skewDataIndex++;
      } else if (su.rs_skewDataIndex == kSkewEstimateFrames) {
        err = estimate_skew(su.rs_skewData, kSkewEstimateFrames, su.scSampFreq, &su.skew);
        su.rs_skewEstimate = su.skew;
        su.rs_skewDataIndex++;
      } else {
        su.skew = su.rs_skewEstimate;
      }
      if (err == -1) {
        su.skew = 0;
        c.lastError = AEC_BAD_PARAMETER_WARNING;
        *rc_ref = -1;
      }
      su.skew /= su.sampFactor * n;
      if (su.skew < 1.0e-3 && su.skew > -1.0e-3) {
        su.resample = kAecFalse;
      } else {
        su.resample = kAecTrue;
      }
      if (su.skew < -0.5f) {
        su.skew = -0.5f;
      } else if (su.skew > 1.0f) {
        su.skew = 1.0f;
      }
    }
  }
  if (c.startup_phase) {
    if (const int rc = flush_pending_farend(su, iss)) return rc;
    if (const int rc = iss.pass_through(n)) return rc;
    if (c.checkBuffSize) {
      c.checkBufSizeCtr++;
      if (c.counter == 0) {
        c.firstVal = c.msInSndCardBuf;
        c.sum = 0;
      }
      double lim = 0.2 * c.msInSndCardBuf;
      if (lim < kSampMsNb) lim = kSampMsNb;
      if (abs(c.firstVal - c.msInSndCardBuf) < lim) {
        c.sum += c.msInSndCardBuf;
        c.counter++;
      } else {
        c.counter = 0;
      }
      if (c.counter * nBlocks10ms >= 6) {
        const int v = (3 * c.sum * su.rate_factor * 8) / (4 * c.counter * kPartLen);
        c.bufSizeStart = v < kMaxBufSizeStart ? v : kMaxBufSizeStart;
        c.checkBuffSize = 0;
      }
      if (c.checkBufSizeCtr * nBlocks10ms > 50) {
        const int v = (c.msInSndCardBuf * su.rate_factor * 3) / 40;
        c.bufSizeStart = v < kMaxBufSizeStart ? v : kMaxBufSizeStart;
        c.checkBuffSize = 0;
      }
    }
    if (!c.checkBuffSize) {
      const int overhead_elements = c.system_delay / kPartLen - c.bufSizeStart;
      if (overhead_elements == 0) {
        c.startup_phase = 0;
      } else if (overhead_elements > 0) {
        far_move_read(c, overhead_elements);
        c.startup_phase = 0;
      }
    }
    return 0;
  }
  if (su.reported_delay_enabled) est_buf_delay_normal(su, c);  // echo_cancellation.c:725-727
  return process_frames_device(su, c, iss, n, c.knownDelay);
}

inline void est_buf_delay_extended(const AecSetup& su, AecCtl& c) {  // EstBufDelayExtended, echo_cancellation.c:869-922
  const int reported_delay = c.msInSndCardBuf * kSampMsNb * su.rate_factor;
  int current_delay = reported_delay - c.system_delay;
  current_delay += kFrameLen * su.rate_factor;
  if (su.skewMode == kAecTrue && su.resample == kAecTrue) current_delay -= kResamplingDelay;  // :884-886
  if (current_delay < kPartLen) current_delay += far_move_read(c, 2) * kPartLen;
  if (c.filtDelay == -1) {
    const double v = 0.5 * current_delay;
    c.filtDelay = (int16_t)(v > 0 ? v : 0);
  } else {
    const int16_t v = (int16_t)(0.95 * c.filtDelay + 0.05 * current_delay);
    c.filtDelay = v > 0 ? v : 0;
  }
  const int delay_difference = c.filtDelay - c.knownDelay;
  if (delay_difference > 384) {
    if (c.lastDelayDiff < 128) {
      c.timeForDelayChange = 0;
    } else {
      c.timeForDelayChange++;
    }
  } else if (delay_difference < 128 && c.knownDelay > 0) {
    if (c.lastDelayDiff > 384) {
      c.timeForDelayChange = 0;
    } else {
      c.timeForDelayChange++;
    }
  } else {
    c.timeForDelayChange = 0;
  }
  c.lastDelayDiff = (int16_t)delay_difference;
  if (c.timeForDelayChange > 25) {
    const int v = (int)c.filtDelay - 256;
    c.knownDelay = v > 0 ? v : 0;
  }
}

// ProcessExtended (echo_cancellation.c:744-814): the trusted-delay build (neither WEBRTC_UNTRUSTED_DELAY nor
// WEBRTC_MAC: kFixedDelayMs 50, kMinTrustedDelayMs 20, kDelayDiffOffsetSamples 0, :70-84).
inline int process_extended_device(AecSetup& su, AecCtl& c, AecIssuer& iss, int n, int16_t reported_delay_ms) {
  const int kFixedDelayMs = 50, kMinTrustedDelayMs = 20, kDelayDiffOffsetSamples = 0;
  reported_delay_ms = reported_delay_ms < kMinTrustedDelayMs ? kMinTrustedDelayMs : reported_delay_ms;
  reported_delay_ms = reported_delay_ms >= kMaxTrustedDelayMs ? kFixedDelayMs : reported_delay_ms;
  c.msInSndCardBuf = reported_delay_ms;
  if (!c.farend_started) return iss.pass_through(n);  // until the far end starts (:768-776)
  if (c.startup_phase) {  // :777-794
    const int startup_size_ms = reported_delay_ms < kFixedDelayMs ? kFixedDelayMs : reported_delay_ms;
    const int overhead_elements = (c.system_delay - startup_size_ms / 2 * su.rate_factor * 8) / kPartLen;
    far_move_read(c, overhead_elements);
    c.startup_phase = 0;
  }
  if (su.reported_delay_enabled) est_buf_delay_extended(su, c);  // echo_cancellation.c:796-798
  const int adjusted = c.knownDelay + kDelayDiffOffsetSamples;
  return process_frames_device(su, c, iss, n, adjusted > 0 ? adjusted : 0);
}

// WebRtcAec_Process checks (echo_cancellation.c:341-375); *rc is the reference's return value.
inline int process_device(AecSetup& su, AecCtl& c, AecIssuer& iss, int n, int msInSndCardBuf, int* rc, int32_t skew = 0) {
  *rc = 0;
  if (msInSndCardBuf < 0) {
    msInSndCardBuf = 0;
    c.lastError = AEC_BAD_PARAMETER_WARNING;
    *rc = -1;
  } else if (msInSndCardBuf > kMaxTrustedDelayMs) {
    c.lastError = AEC_BAD_PARAMETER_WARNING;
    *rc = -1;
  }
  if (su.extended) return process_extended_device(su, c, iss, n, (int16_t)msInSndCardBuf);  // :377-394
  return process_normal_device(su, c, iss, n, (int16_t)msInSndCardBuf, skew, rc);
}

// ------------------------------------------------------------ list calls (AspAecBatch_RunList)
// Where the descriptors of a list call go: `d` is frame `frame` (counted from the launch's first) of entry `entry`.
struct AecListSink {
  virtual int step(int entry, int frame, const AecListStep& d) = 0;

 protected:
  ~AecListSink() = default;
};

// The issuer of the planning step: what one BufferFarend + Process pair of one stream issues, as one descriptor.
struct AecListRecorder final : AecIssuer {
  AecListStep d;
  int far_recorded = 0;
  void begin() {
    memset(&d, 0, sizeof d);
    far_recorded = 0;
  }
  int farend(const float*, const FarOps& ops) override {
    if (far_recorded++ != 0) return aec_refuse("list call: a far-end call of more than three partitions");
    d.far = ops;
    return 0;
  }
  int process(int, const ProcOps& ops, const float* far_src, const FarOps&, const AgnOps* agn, int) override {
    if (far_src != nullptr || agn != nullptr || ops.agnostic || ops.spectra || ops.num_high)
      return aec_refuse("list call: a Process descriptor outside per-stream control");
    d.mode = 1;
    d.ops = ops;
    return 0;
  }
  int pass_through(int) override {
    d.mode = 0;
    return 0;
  }
  int delay(const DelayOps&) override { return aec_refuse("per-stream control runs no delay estimator"); }
  int resample(const float**, int, int, float, float) override {
    return aec_refuse("skew compensation runs on plain launches only");
  }
};

// The planning step of a list call.  ctl[i] is the control plane of entry i's stream -- the caller hands in copies
// and commits them once the launch is enqueued, so a refusal leaves the batch as it was.  Walks the entries and, of
// each, frames frame0 .. min(counts[i], frame0 + frames) - 1 in order: WebRtcAec_BufferFarend, then WebRtcAec_Process
// with the entry's reported delay ms[i], recorded as one descriptor and handed to `sink`; status[i] (may be null)
// collects the OR of the reference's return values.
inline int plan_list(AecSetup& su, AecCtl* ctl, const int32_t* counts, int n, int frame0, int frames, int nrOfSamples,
                     const int16_t* ms, int32_t* status, AecListSink& sink) {
  static const float kNoSamples = 0.f;  // the control functions take the far frame's address and never read it
  AecListRecorder rec;
  for (int i = 0; i < n; ++i) {
    const int end = counts[i] < frame0 + frames ? counts[i] : frame0 + frames;
    for (int f = frame0; f < end; ++f) {
      rec.begin();
      if (const int err = buffer_farend_device(su, ctl[i], rec, &kNoSamples, nrOfSamples)) return err;
      int rc = 0;
      if (const int err = process_device(su, ctl[i], rec, nrOfSamples, ms[i], &rc)) return err;
      if (status) status[i] |= rc;
      if (const int err = sink.step(i, f - frame0, rec.d)) return err;
    }
  }
  return 0;
}

}  // namespace aspaec
#pragma GCC visibility pop
