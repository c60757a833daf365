// aec_api.hip -- host side of include/asp_aec.h: constant tables, the batch handle and its device
// resources, the issuer that carries the control plane's launch descriptors (aec_layout.h: FarOps /
// ProcOps) to the device, and the reference's per-stream WebRtcAec_* symbols as a batch of one.  The
// reference's integer control plane itself is host-only code in aec_control.h; it runs once per call
// for the whole batch (or once per stream under per-stream control); all sample and spectrum data
// stays in HBM.  No CPU fallback.
#include <hip/hip_runtime.h>

#include "api_common.h"

#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "aec_control.h"
#include "aec_layout.h"
#include "asp_aec.h"
#include "asp_ns.h"
#include "handoff_host.h"

using namespace aspaec;

namespace aspaec {
hipError_t launch_aec_farend(float* state, float* far_ring, const AecTables* T, const float* farend,
                             int num_streams, const FarOps& ops, hipStream_t s, int stream0 = 0,
                             int stream_end = -1, int num_part = kNumPartNormal);
hipError_t launch_aec_process(float* state, float* far_ring, const AecTables* T,
                              const float* nearend, float* out, int num_streams, int nrOfSamples,
                              const ProcOps& ops, const float* farend, const FarOps& fops,
                              const float* near_high, float* out_high, float* metrics,
                              hipStream_t s, unsigned long long* stamps = nullptr, int stream0 = 0,
                              int stream_end = -1, int num_part = kNumPartNormal, float* spectra = nullptr,
                              const DelayBlock* dblocks = nullptr);
hipError_t launch_aec_process_flow(float* state, float* far_ring, const AecTables* T, int num_streams, int nrOfSamples,
                                   const AecFlowStep* descs, int steps, unsigned* seq, unsigned* abort_w, unsigned want,
                                   int num_part, hipStream_t s, DelayBlock* est, unsigned* bits, bool agn);
hipError_t launch_aec_process_agn(float* state, float* far_ring, const AecTables* T, const float* nearend, float* out,
                                  int num_streams, int nrOfSamples, const ProcOps& ops, const float* farend, const FarOps& fops,
                                  DelayBlock* dblocks, const AgnOps& agn, hipStream_t s, int stream0, int stream_end,
                                  int num_part);
hipError_t launch_aec_delay_bits(DelayBlock* blocks, const unsigned* bits, int num_streams, int npending, int logging,
                                 hipStream_t s);
hipError_t launch_aec_farend_v(float* state, float* far_ring, const AecTables* T, const float* farend, int num_streams,
                               const FarOps* vfar, int nrOfSamples, int num_part, hipStream_t s);
hipError_t launch_aec_process_v(float* state, float* far_ring, const AecTables* T, const float* nearend, float* out,
                                int num_streams, int nrOfSamples, const AecStreamStep* vdesc, int num_part, hipStream_t s);
hipError_t launch_aec_list(float* state, float* far_ring, const AecTables* T, const float* farend, const float* nearend,
                           float* out, int num_streams, int nrOfSamples, int n, const AecListEntry* list,
                           const AecListStep* descs, int stride, const ProcOps& batch_ops, int num_part, hipStream_t s);
hipError_t launch_aec_delay(DelayBlock* blocks, const float* spectra, int num_streams, const DelayOps& ops,
                            hipStream_t s);
hipError_t launch_aec_resample(float* rs_buffer, const float* farend, float* out, int num_streams, int size, int size_out,
                               float be, float position, hipStream_t s);
hipError_t launch_aec_rdft128(const float* src, float* dst, int isgn, int count, const AecTables* T,
                              hipStream_t s);
}  // namespace aspaec

namespace {

#define aec_fail(...) asp_fail("asp_aec", __VA_ARGS__)
#define AEC_TRY(x) ASP_TRY("asp_aec", x)

// ------------------------------------------------------------------ tables
// NOTE: C++ translation unit; every libm call casts to double explicitly so the arithmetic is
// that of the reference's C (see ns_api.hip).
unsigned bitrev(unsigned x, int bits) {
  unsigned r = 0;
  for (int b = 0; b < bits; ++b) r |= ((x >> b) & 1u) << (bits - 1 - b);
  return r;
}

float via_text(double v, int decimals) {  // a table frozen as '%.<d>f' text and re-read as float
  char buf[48];
  snprintf(buf, sizeof buf, "%.*f", decimals, v);
  return strtof(buf, nullptr);
}

void build_tables(AecTables* T) {
  memset(T, 0, sizeof *T);
  // Ooura makewt / makect for n = 128, the code the reference's frozen rdft_w came from
  // (aec_rdft.c:29-49; utility/fft4g.c:642-690 is the same code)
  float tmp[32];
  const int nw = 32, nwh = 16, nc = 32, nch = 16;
  float delta = (float)atan((double)1.0f) / nwh;
  tmp[0] = 1;
  tmp[1] = 0;
  tmp[nwh] = (float)cos((double)(delta * nwh));
  tmp[nwh + 1] = tmp[nwh];
  for (int j = 2; j < nwh; j += 2) {
    const float x = (float)cos((double)(delta * j));
    const float y = (float)sin((double)(delta * j));
    tmp[j] = x;
    tmp[j + 1] = y;
    tmp[nw - j] = y;
    tmp[nw - j + 1] = x;
  }
  for (int j = 0; j < 16; ++j) {
    const unsigned r = bitrev((unsigned)j, 4);
    T->w[2 * j] = tmp[2 * r];
    T->w[2 * j + 1] = tmp[2 * r + 1];
  }
  delta = (float)atan((double)1.0f) / nch;
  T->w[32] = (float)cos((double)(delta * nch));
  T->w[32 + nch] = 0.5f * T->w[32];
  for (int j = 1; j < nch; j++) {
    T->w[32 + j] = 0.5f * (float)cos((double)(delta * j));
    T->w[32 + nc - j] = 0.5f * (float)sin((double)(delta * j));
  }
  {
    // the frozen text differs from the evaluation above by one unit in the last place at eight
    // entries (data of the reference, aec_rdft.c:32-49)
    static const signed char nudge[8][2] = {{4, 1}, {7, 1}, {20, 1}, {27, 1},
                                            {40, 1}, {41, -1}, {42, 1}, {47, 1}};
    for (int k = 0; k < 8; ++k) {
      int32_t bits;
      memcpy(&bits, &T->w[nudge[k][0]], sizeof bits);
      bits += nudge[k][1];
      memcpy(&T->w[nudge[k][0]], &bits, sizeof bits);
    }
  }
  for (int k1 = 0; k1 < 16; k1 += 2) {  // rdft_wk3ri_first / _second (aec_rdft.c:50-61)
    const int k2 = 2 * k1;
    const float wk2r = T->w[k1], wk2i = T->w[k1 + 1];
    float wk1r = T->w[k2], wk1i = T->w[k2 + 1];
    T->wk3a[k1] = wk1r - 2 * wk2i * wk1i;
    T->wk3a[k1 + 1] = 2 * wk2i * wk1r - wk1i;
    wk1r = T->w[k2 + 2];
    wk1i = T->w[k2 + 3];
    T->wk3b[k1] = wk1r - 2 * wk2r * wk1i;
    T->wk3b[k1 + 1] = 2 * wk2r * wk1r - wk1i;
  }
  for (int k = 0; k <= 64; ++k) {  // aec_core.c:50-98
    T->hann[k] = via_text(sin(M_PI * (double)k / 128.0), 14);
    T->weight[k] = k == 0 ? 0.f : via_text(0.3 * sqrt((double)(k - 1) / 63.0) + 0.1, 4);
    T->odrive[k] = via_text(sqrt((double)k / 64.0) + 1.0, 4);
  }
  for (int j = 0; j < 64; ++j) T->exp2_64[j] = exp2((double)j / 64.0);
  uint32_t a = 1, c = 0;  // WebRtcSpl_RandU jump-ahead (randomization_functions.c:93-100)
  for (int k = 0; k < 64; ++k) {
    c = c * 69069u + 1u;
    a = a * 69069u;
    T->lcg_a[k] = a;
    T->lcg_c[k] = c;
  }
}

}  // namespace

int aspaec::aec_refuse(const char* what) { return aec_fail(ASP_ERR_STATE, what); }

// The batch: one setup, the control plane of the batch fed in lock-step (`ctl`) or -- once a caller drives streams
// apart (AspAecBatch_ProcessV / _InitStream) -- one per stream (`per`), and the device resources.  The control
// functions (aec_control.h) run on the setup and ONE AecCtl and issue their device work through a DeviceIssuer
// (below) that the entry point builds for the call.
struct AspAecBatch {
  AecSetup su;
  AecCtl ctl;
  std::vector<AecCtl> per;  // empty while the batch runs in lock-step
  int S = 0, device = 0;    // device < 0: control-only handle (AspAecBatch_CreateControlOnly), no device resources
  hipStream_t stream = nullptr;
  bool own_stream = false;
  float* state = nullptr;     // [S][AecRows(num_part).state_dwords]
  // delay estimation (set_config delay_logging) and the delay-agnostic mode (WebRtcAec_enable_reported_delay 0):
  // per-stream estimator blocks and the power spectra the process kernel leaves for them
  DelayBlock* dblocks = nullptr;  // [S]
  float* spectra = nullptr;       // [S][kSpecBlocks][kSpecDwords]
  float* rs_buffer = nullptr;  // [S][kResamplerBufferSize]
  float* stage_rs = nullptr;   // [S][kResamplerBufferSize]: the resampled far frame of the call in flight
  float* far_ring = nullptr;  // [kFarSlots][S][kFarSlotDwords]
  AecTables* tables = nullptr;
  float *stage_far = nullptr, *stage_near = nullptr, *stage_out = nullptr;  // [S][160]
  float *stage_near_h = nullptr, *stage_out_h = nullptr;                    // [S][160]
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // two launch chains over the two halves of the batch (the K-step path, AspAecBatch_TimedSteps): streams are
  // independent, so half B's step k may still run while half A's step k + 1 starts -- the load burst of one
  // overlaps the transforms of the other
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // Hand-off build of the multi-frame entry points (Run on device buffers, TimedSteps; aec_kernels.hip,
  // AecFlowArgs; handoff.h): the Process launches are not issued one by one but recorded as descriptors; up to
  // kHandoffMaxSteps of them go into ONE launch (grid y = step), in which a per-stream step counter in memory
  // orders a stream's consecutive steps.  -1 = default (on), 0 = off, 1 = on.
  int flow = -1;
  int flow_slot = 0;                         // ring of descriptor arrays: host (pinned) and device copies
  unsigned char* flow_host = nullptr;        // [kAecFlowSlots][kHandoffMaxSteps] AecFlowStep, or AecFlowStepAgn in the delay-agnostic mode
  unsigned char* flow_dev = nullptr;
  hipEvent_t flow_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // slot i's launch has consumed its descriptors
  HandoffSync sync;
  unsigned* flow_bits = nullptr;             // delay logging: [S][kFlowBitsBlocks][2] binary spectra of the recorded steps' blocks
  // Per-stream control: the launch descriptors of a call recorded per stream and read by the kernels from device memory
  AecStreamStep* vproc_host = nullptr;       // [S], pinned: this call's Process descriptor of every stream
  AecStreamStep* vproc_dev = nullptr;
  FarOps* vfar_host = nullptr;               // [S], pinned: this call's far-end work of every stream
  FarOps* vfar_dev = nullptr;
  hipEvent_t vev = nullptr;                  // the last per-stream launch has read its descriptors
  // List calls (AspAecBatch_RunList): a ring of kAecListSlots slots, each one launch's entries [S] and descriptors
  // [S][kAecListMaxFrames]; allocated by the first list call
  unsigned char* list_host = nullptr;        // pinned
  unsigned char* list_dev = nullptr;
  hipEvent_t list_ev[kAecListSlots] = {};    // slot i's launch has read its descriptors
  int list_slot = 0;
  // echo metrics (aec_core.c:548-770): [S][kMetDwords], updated by the kernel when metricsMode is on
  float* metrics = nullptr;
};


namespace {
constexpr int kAecFlowSlots = 4;
static_assert(kFlowBitsBlocks >= 4 * kHandoffMaxSteps, "a step has at most four blocks");
constexpr size_t kAecFlowElem = sizeof(AecFlowStepAgn);  // a slot holds kHandoffMaxSteps elements of either type

bool control_only(const AspAecBatch* b) { return b->device < 0; }
bool vmode(const AspAecBatch* b) { return !b->per.empty(); }
// The control plane of stream s; and the one that the batch-level accessors mean (GetControl, get_error_code, the
// reference's error codes, the WebRtcAec_* core getters): the batch's -- with per-stream control, stream 0's.
const AecCtl& ctl_of(const AspAecBatch* b, int s) { return vmode(b) ? b->per[(size_t)s] : b->ctl; }
AecCtl& ctl0(AspAecBatch* b) { return const_cast<AecCtl&>(ctl_of(b, 0)); }
int set_error(AspAecBatch* b, int code) {  // the reference's lastError = code; return -1
  ctl0(b).lastError = code;
  return -1;
}

// The delay-agnostic mode in one launch per call (aec_process_agn_kernel): one band, no echo metrics, the whole batch on
// one control plane.  ASP_AEC_AGN_FUSED=0 keeps the launch-per-sub-frame form (the A / B switch).
bool agn_fusable(const AspAecBatch* b) {
  static const int env = [] {
    const char* e = getenv("ASP_AEC_AGN_FUSED");
    return e ? atoi(e) : 1;
  }();
  return env != 0 && b->su.num_high == 0 && !b->su.metricsMode;
}

// The hand-off build serves one band without skew compensation and echo metrics: the plain configuration, delay
// logging (the estimator's launch follows each process launch) and the fused delay-agnostic mode.  Per-stream
// control has one far-end and one Process launch per call instead.
bool aec_flow_applies(const AspAecBatch* b, int steps) {
  const bool on = b->flow < 0 ? handoff_env_default("ASP_AEC_FLOW") : b->flow != 0;
  return on && steps >= 2 && !vmode(b) && b->su.num_high == 0 && !b->su.metricsMode &&
         (b->su.reported_delay_enabled || agn_fusable(b)) && !b->su.skewMode;
}
int aec_flow_resources(AspAecBatch* b) {
  if (b->su.delay_logging && b->flow_bits == nullptr)
    AEC_TRY(hipMalloc((void**)&b->flow_bits, (size_t)b->S * kFlowBitsBlocks * 2 * sizeof(unsigned)));
  if (b->sync.seq) return 0;
  AEC_TRY(b->sync.ensure(b->S, b->stream));
  AEC_TRY(hipHostMalloc((void**)&b->flow_host, kAecFlowElem * kAecFlowSlots * kHandoffMaxSteps, hipHostMallocDefault));
  AEC_TRY(hipMalloc((void**)&b->flow_dev, kAecFlowElem * kAecFlowSlots * kHandoffMaxSteps));
  for (int i = 0; i < kAecFlowSlots; ++i) AEC_TRY(hipEventCreateWithFlags(&b->flow_ev[i], hipEventDisableTiming));
  b->flow_slot = 0;
  return 0;
}
// after the batch's stream has been synchronised: did a hand-off wait time out?
int aec_flow_check(AspAecBatch* b) {
  bool timed_out = false;
  AEC_TRY(b->sync.check(b->S, &timed_out));
  if (!timed_out) return 0;
  return aec_fail(ASP_ERR_HIP, "AEC hand-off wait timed out: frame steps were skipped, re-initialise the batch");
}

// Where the device work of a control step goes.  The entry point that knows the situation builds one on its stack:
//   kNone     a control-only handle (whatever mode is asked for): nothing is issued
//   kLaunch   plain launches on the batch's stream, or one per half of the batch on two chains (`side`)
//   kHandoff  the hand-off build: Process steps are recorded and go out kHandoffMaxSteps to a launch; whatever else
//             is issued follows the recorded steps.  finish() issues the rest; a recording left behind is dropped.
//   kStream   per-stream control: stream s's descriptors of the call, which one launch for all streams reads
struct DeviceIssuer final : AecIssuer {
  enum Mode { kNone, kLaunch, kHandoff, kStream };
  AspAecBatch* const b;
  const Mode mode;
  const int s;
  const float *near = nullptr, *near_high = nullptr;  // device buffers of the Process call in flight
  float *out = nullptr, *out_high = nullptr;
  hipStream_t side = nullptr;            // kLaunch: the second chain
  unsigned long long* const stamps;      // kLaunch: diagnostic only (AspAecBatch_DebugStamps)
  int far_recorded = 0;                  // kStream: far-end descriptors of this call
  int flow_n = 0, flow_nr = 0;           // kHandoff: descriptors recorded so far; samples per call of the recording
  int flow_blocks = 0;                   // blocks of the recording so far (their spectra wait for aec_delay_bits_kernel)
  bool flow_agn = false;                 // the recording's element type

  DeviceIssuer(AspAecBatch* b_, Mode m, int s_ = 0, unsigned long long* stamps_ = nullptr)
      : b(b_), mode(control_only(b_) ? kNone : m), s(s_), stamps(stamps_) {
    agn_fused = (mode == kLaunch || mode == kHandoff) && stamps == nullptr && agn_fusable(b);
  }

  // one launch, or one per half on the two chains (time stamps: the first half's)
  template <class F>
  int on_chains(F launch) {
    const int half = side ? ((b->S / 2 + 3) / 4) * 4 : -1;
    AEC_TRY(launch(b->stream, 0, half, stamps));
    if (side) AEC_TRY(launch(side, half, b->S, (unsigned long long*)nullptr));
    return 0;
  }

  int farend(const float* far, const FarOps& ops) override {
    switch (mode) {
      case kNone: return 0;
      case kStream:  // one descriptor: nothing is deferred
        if (far_recorded++ != 0) AEC_TRY(hipErrorUnknown);
        b->vfar_host[s] = ops;
        return 0;
      case kHandoff:
        if (const int rc = finish()) return rc;
        [[fallthrough]];
      case kLaunch: break;
    }
    return on_chains([&](hipStream_t st, int s0, int s1, unsigned long long*) {
      return launch_aec_farend(b->state, b->far_ring, b->tables, far, b->S, ops, st, s0, s1, b->su.num_part);
    });
  }

  int process(int n, const ProcOps& ops, const float* far_src, const FarOps& fops, const AgnOps* agn, int sub) override {
    switch (mode) {
      case kNone: return ops.agnostic ? aec_fail(ASP_ERR_STATE, "the delay-agnostic mode needs the device") : 0;
      case kStream:
        if (far_src != nullptr) AEC_TRY(hipErrorUnknown);  // a fused far end
        b->vproc_host[s].mode = 1;
        b->vproc_host[s].ops = ops;
        return 0;
      case kHandoff: return record(n, ops, far_src, fops, agn);
      case kLaunch: break;
    }
    const int np = b->su.num_part;
    if (agn)
      return on_chains([&](hipStream_t st, int s0, int s1, unsigned long long*) {
        return launch_aec_process_agn(b->state, b->far_ring, b->tables, near, out, b->S, n, ops, far_src, fops, b->dblocks,
                                      *agn, st, s0, s1, np);
      });
    const size_t off = sub > 0 ? (size_t)kFrameLen * sub : 0;
    return on_chains([&](hipStream_t st, int s0, int s1, unsigned long long* stamps_) {
      return launch_aec_process(b->state, b->far_ring, b->tables, near + off, out + off, b->S, n, ops, far_src, fops,
                                near_high ? near_high + off : nullptr, out_high ? out_high + off : nullptr,
                                b->su.metricsMode ? b->metrics : nullptr, st, sub > 0 ? nullptr : stamps_, s0, s1, np,
                                b->spectra, b->dblocks);
    });
  }

  int pass_through(int n) override {
    switch (mode) {
      case kNone: return 0;
      case kStream:
        b->vproc_host[s].mode = 0;  // the kernel copies this stream's near end
        return 0;
      case kHandoff:
        if (const int rc = finish()) return rc;
        [[fallthrough]];
      case kLaunch: break;
    }
    const size_t bytes = (size_t)b->S * n * sizeof(float);
    if (near != out) AEC_TRY(hipMemcpyAsync(out, near, bytes, hipMemcpyDeviceToDevice, b->stream));
    if (b->su.num_high > 0 && near_high != out_high)
      AEC_TRY(hipMemcpyAsync(out_high, near_high, bytes, hipMemcpyDeviceToDevice, b->stream));
    return 0;
  }

  int delay(const DelayOps& d) override {
    switch (mode) {
      case kNone: return d.control ? aec_fail(ASP_ERR_STATE, "the delay-agnostic mode needs the device") : 0;
      case kStream: return aec_fail(ASP_ERR_STATE, "per-stream control runs no delay estimator");
      case kHandoff:
        if (!d.control) return 0;  // the estimator's share of the recorded steps: record() counts it, finish() issues it
        if (const int rc = finish()) return rc;
        [[fallthrough]];
      case kLaunch: break;
    }
    AEC_TRY(launch_aec_delay(b->dblocks, b->spectra, b->S, d, b->stream));
    return 0;
  }

  int resample(const float** far, int n, int n_out, float be, float position) override {
    switch (mode) {
      case kNone: return 0;
      case kLaunch: break;
      default: return aec_fail(ASP_ERR_STATE, "skew compensation runs on plain launches only");
    }
    AEC_TRY(launch_aec_resample(b->rs_buffer, *far, b->stage_rs, b->S, n, n_out, be, position, b->stream));
    *far = b->stage_rs;
    return 0;
  }

  // kHandoff: issue the recorded steps as one launch
  int finish() {
    if (flow_n == 0) return 0;
    const int slot = b->flow_slot;
    unsigned char* h = b->flow_host + (size_t)slot * kHandoffMaxSteps * kAecFlowElem;
    unsigned char* d = b->flow_dev + (size_t)slot * kHandoffMaxSteps * kAecFlowElem;
    const int n = flow_n;
    flow_n = 0;
    const bool agn = flow_agn;
    AEC_TRY(hipMemcpyAsync(d, h, (agn ? sizeof(AecFlowStepAgn) : sizeof(AecFlowStep)) * n, hipMemcpyHostToDevice, b->stream));
    const int blocks = flow_blocks;  // > 0: delay logging is on
    flow_blocks = 0;
    AEC_TRY(launch_aec_process_flow(b->state, b->far_ring, b->tables, b->S, flow_nr, reinterpret_cast<const AecFlowStep*>(d), n,
                                    b->sync.seq, b->sync.abort, b->sync.count, b->su.num_part, b->stream,
                                    (agn || blocks > 0) ? b->dblocks : nullptr, blocks > 0 ? b->flow_bits : nullptr, agn));
    // the estimator's share of these steps (aec_core.c:1191-1203): one launch for all their blocks, from the binary
    // spectra the process kernel left
    if (blocks > 0) AEC_TRY(launch_aec_delay_bits(b->dblocks, b->flow_bits, b->S, blocks, 1, b->stream));
    AEC_TRY(hipEventRecord(b->flow_ev[slot], b->stream));
    b->sync.enqueued(n);
    b->flow_slot = (slot + 1) % kAecFlowSlots;
    // the next slot's previous launch must have read its descriptors before they are overwritten
    AEC_TRY(hipEventSynchronize(b->flow_ev[b->flow_slot]));
    return 0;
  }
  int record(int n, const ProcOps& ops, const float* far_src, const FarOps& fops, const AgnOps* agn) {
    if (flow_n > 0 && (flow_nr != n || flow_agn != (agn != nullptr))) {  // a launch carries calls of one length and one kind
      if (const int rc = finish()) return rc;
    }
    flow_nr = n;
    flow_agn = agn != nullptr;
    unsigned char* slot_base = b->flow_host + (size_t)b->flow_slot * kHandoffMaxSteps * kAecFlowElem;
    const int idx = flow_n++;
    AecFlowStepAgn* sa = agn ? reinterpret_cast<AecFlowStepAgn*>(slot_base) + idx : nullptr;
    AecFlowStep& st = agn ? sa->step : reinterpret_cast<AecFlowStep*>(slot_base)[idx];
    if (agn) sa->agn = *agn;
    memset(&st, 0, sizeof st);
    st.ops = ops;
    st.fops = fops;
    st.farend = far_src;
    st.nearend = near;
    st.out = out;
    st.spec_base = -1;
    if (b->su.delay_logging && agn == nullptr) {  // (the delay-agnostic mode runs the estimator in the process wave)
      st.spec_base = flow_blocks;
      for (int j = 0; j < ops.nsub; ++j) flow_blocks += ops.sub[j].nblocks;  // <= 4 per step, kFlowBitsBlocks = 4 * kHandoffMaxSteps
    }
    return flow_n == kHandoffMaxSteps ? finish() : 0;
  }
};

// WebRtc_InitDelayEstimatorFarend / WebRtc_InitDelayEstimator and the AecCore fields around them (aec_core.c:1502-1516,
// delay_estimator_wrapper.c:175-191, 305-322, delay_estimator.c:303-307, 476-498) for every stream.  The lookahead
// is not part of Init: a stream keeps what Create set or the agnostic mode's soft resets left (as the reference does).
void init_delay_state(AspAecDelayState* d, int lookahead, int allowed_offset) {
  memset(d, 0, sizeof *d);
  d->lookahead = lookahead;
  d->allowed_offset = allowed_offset;
  for (int i = 0; i <= ASP_AEC_DELAY_HISTORY; ++i) d->mean_bit_counts[i] = (20 << 9);
  d->minimum_probability = 32 << 9;
  d->last_delay_probability = 32 << 9;
  d->last_delay = -2;
  d->last_candidate_delay = -2;
  d->compare_delay = ASP_AEC_DELAY_HISTORY;
  d->previous_delay = -2;
  d->shift_offset = 5;  // kInitialShiftOffset, aec_core.c:102
}
int init_delay_device(AspAecBatch* b, AspDeviceScope& dev_scope_) {
  std::vector<DelayBlock> all((size_t)b->S);
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  AEC_TRY(hipMemcpy(all.data(), b->dblocks, all.size() * sizeof(DelayBlock), hipMemcpyDeviceToHost));
  for (auto& d : all) {
    const int lookahead = d.s.lookahead;
    memset(&d, 0, sizeof d);
    init_delay_state(&d.s, lookahead, kNumPartNormal / 2);  // WebRtc_set_allowed_offset(num_partitions / 2), aec_core.c:1529
  }
  AEC_TRY(hipMemcpy(b->dblocks, all.data(), all.size() * sizeof(DelayBlock), hipMemcpyHostToDevice));
  return 0;
}

// InitMetrics (aec_core.c:548-583) for every stream, ordered on the batch's stream.
int init_metrics_device(AspAecBatch* b, AspDeviceScope& dev_scope_) {
  AspAecMetricsState m;
  memset(&m, 0, sizeof m);
  AspAecPowerLevel* lv[4] = {&m.farlevel, &m.nearlevel, &m.linoutlevel, &m.nlpoutlevel};
  for (AspAecPowerLevel* l : lv) l->minlevel = 1E17f;
  AspAecStats* st[4] = {&m.erl, &m.erle, &m.aNlp, &m.rerl};
  for (AspAecStats* s : st) {
    s->instant = s->average = s->max = s->himean = -100;  // kOffsetLevel
    s->min = 100;
  }
  static_assert(sizeof(AspAecMetricsState) == 65 * 4 && sizeof(AspAecMetricsState) <= kMetDwords * 4, "metrics image");
  std::vector<float> all((size_t)b->S * kMetDwords, 0.f);
  for (int s = 0; s < b->S; ++s) memcpy(all.data() + (size_t)s * kMetDwords, &m, sizeof m);
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  AEC_TRY(hipMemcpy(b->metrics, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
  return 0;
}

int state_dwords(const AspAecBatch* b) { return AecRows(b->su.num_part).state_dwords; }
size_t state_bytes(const AspAecBatch* b) { return (size_t)b->S * state_dwords(b) * sizeof(float); }
size_t far_bytes(const AspAecBatch* b) {
  return (size_t)kFarSlots * b->S * kFarSlotDwords * sizeof(float);
}

// ---- AspAecState <-> device block
void pack_stream(int num_part, const AecCtl& c, const AspAecState* s, float* blk) {
  const AecRows rw(num_part);
  const int kNumPart = rw.NP, R_XF_IM = rw.R_XF_IM, R_WF_RE = rw.R_WF_RE, R_WF_IM = rw.R_WF_IM, R_XFW = rw.R_XFW;
  memset(blk, 0, rw.state_dwords * sizeof(float));
  float* rows = blk + kOffRows;
  auto put_row = [&](int r, const float* src) {
    memcpy(rows + r * kRowS, src, 64 * sizeof(float));
    blk[kOffC64 + r] = src[64];
  };
  put_row(R_XPOW, s->xPow);
  put_row(R_DPOW, s->dPow);
  put_row(R_DMINPOW, s->dMinPow);
  put_row(R_DINITMINPOW, s->dInitMinPow);
  put_row(R_SX, s->sx);
  put_row(R_SD, s->sd);
  put_row(R_SE, s->se);
  {
    float tmp[4][65];
    for (int i = 0; i < 65; ++i) {
      tmp[0][i] = s->sde[i][0];
      tmp[1][i] = s->sde[i][1];
      tmp[2][i] = s->sxd[i][0];
      tmp[3][i] = s->sxd[i][1];
    }
    put_row(R_SDE_RE, tmp[0]);
    put_row(R_SDE_IM, tmp[1]);
    put_row(R_SXD_RE, tmp[2]);
    put_row(R_SXD_IM, tmp[3]);
  }
  for (int a = 0; a < kNumPart; ++a) {  // logical age a: canonical (c + a) % NP -> physical (h + a) % NP
    const int pc = (s->xfBufBlockPos + a) % kNumPart, ph = (c.xf_pos + a) % kNumPart;
    put_row(R_XF_RE + ph, s->xfBuf[0] + pc * 65);
    put_row(R_XF_IM + ph, s->xfBuf[1] + pc * 65);
  }
  for (int i = 0; i < kNumPart; ++i) {
    put_row(R_WF_RE + i, s->wfBuf[0] + i * 65);
    put_row(R_WF_IM + i, s->wfBuf[1] + i * 65);
  }
  {
    // canonical partition a >= 1 holds the block of age a - 1 (aec_core.c:1079-1081); physical
    // age g sits at (xfw_head + g) % 32: all 32 blocks of history whatever the filter length, as the
    // reference shifts them (aec_core.c:1079-1081)
    const float* raw = &s->xfwBuf[0][0];
    for (int a = 1; a < kNumPartMax; ++a) {
      const int ph = (c.xfw_head + a - 1) % kNumPartMax;
      put_row(R_XFW + 2 * ph, raw + a * 130);
      put_row(R_XFW + 2 * ph + 1, raw + a * 130 + 65);
    }
  }
  memcpy(blk + kOffDBuf, s->dBuf, 64 * sizeof(float));
  memcpy(blk + kOffEBuf, s->eBuf, 64 * sizeof(float));
  memcpy(blk + kOffOutBuf, s->outBuf, 64 * sizeof(float));
  memcpy(blk + kOffDBufH, s->dBufH, 64 * sizeof(float));
  float* sc = blk + kOffScalars;
  int32_t* sci = reinterpret_cast<int32_t*>(sc);
  sc[S_HNLFBMIN] = s->hNlFbMin;
  sc[S_HNLFBLOCALMIN] = s->hNlFbLocalMin;
  sc[S_HNLXDAVGMIN] = s->hNlXdAvgMin;
  sc[S_OVERDRIVE] = s->overDrive;
  sc[S_OVERDRIVESM] = s->overDriveSm;
  sci[S_HNLNEWMIN] = s->hNlNewMin;
  sci[S_HNLMINCTR] = s->hNlMinCtr;
  sci[S_DELAYIDX] = s->delayIdx;
  sci[S_STNEARSTATE] = s->stNearState;
  sci[S_ECHOSTATE] = s->echoState;
  sci[S_DIVERGESTATE] = s->divergeState;
  sci[S_NOISEESTCTR] = s->noiseEstCtr;
  sci[S_DELAYESTCTR] = s->delayEstCtr;
  reinterpret_cast<uint32_t*>(sc)[S_SEED] = s->seed;
}

void unpack_stream(int num_part, const AecCtl& c, const float* blk, AspAecState* s) {
  const AecRows rw(num_part);
  const int kNumPart = rw.NP, R_XF_IM = rw.R_XF_IM, R_WF_RE = rw.R_WF_RE, R_WF_IM = rw.R_WF_IM, R_XFW = rw.R_XFW;
  memset(s, 0, sizeof *s);
  const float* rows = blk + kOffRows;
  auto get_row = [&](int r, float* dst) {
    memcpy(dst, rows + r * kRowS, 64 * sizeof(float));
    dst[64] = blk[kOffC64 + r];
  };
  get_row(R_XPOW, s->xPow);
  get_row(R_DPOW, s->dPow);
  get_row(R_DMINPOW, s->dMinPow);
  get_row(R_DINITMINPOW, s->dInitMinPow);
  get_row(R_SX, s->sx);
  get_row(R_SD, s->sd);
  get_row(R_SE, s->se);
  {
    float tmp[4][65];
    get_row(R_SDE_RE, tmp[0]);
    get_row(R_SDE_IM, tmp[1]);
    get_row(R_SXD_RE, tmp[2]);
    get_row(R_SXD_IM, tmp[3]);
    for (int i = 0; i < 65; ++i) {
      s->sde[i][0] = tmp[0][i];
      s->sde[i][1] = tmp[1][i];
      s->sxd[i][0] = tmp[2][i];
      s->sxd[i][1] = tmp[3][i];
    }
  }
  for (int i = 0; i < kNumPart; ++i) {
    get_row(R_XF_RE + i, s->xfBuf[0] + i * 65);
    get_row(R_XF_IM + i, s->xfBuf[1] + i * 65);
    get_row(R_WF_RE + i, s->wfBuf[0] + i * 65);
    get_row(R_WF_IM + i, s->wfBuf[1] + i * 65);
  }
  s->xfBufBlockPos = c.xf_pos;
  {
    float* raw = &s->xfwBuf[0][0];
    for (int a = 0; a < kNumPartMax; ++a) {
      const int ph = (c.xfw_head + (a == 0 ? 0 : a - 1)) % kNumPartMax;
      get_row(R_XFW + 2 * ph, raw + a * 130);
      get_row(R_XFW + 2 * ph + 1, raw + a * 130 + 65);
    }
  }
  memcpy(s->dBuf, blk + kOffDBuf, 64 * sizeof(float));
  memcpy(s->dBuf + 64, blk + kOffDBuf, 64 * sizeof(float));  // the copy left by aec_core.c:1070
  memcpy(s->eBuf, blk + kOffEBuf, 64 * sizeof(float));
  memcpy(s->eBuf + 64, blk + kOffEBuf, 64 * sizeof(float));
  memcpy(s->outBuf, blk + kOffOutBuf, 64 * sizeof(float));
  memcpy(s->dBufH, blk + kOffDBufH, 64 * sizeof(float));
  memcpy(s->dBufH + 64, blk + kOffDBufH, 64 * sizeof(float));  // the copy left by aec_core.c:1076
  const float* sc = blk + kOffScalars;
  const int32_t* sci = reinterpret_cast<const int32_t*>(sc);
  s->hNlFbMin = sc[S_HNLFBMIN];
  s->hNlFbLocalMin = sc[S_HNLFBLOCALMIN];
  s->hNlXdAvgMin = sc[S_HNLXDAVGMIN];
  s->overDrive = sc[S_OVERDRIVE];
  s->overDriveSm = sc[S_OVERDRIVESM];
  s->hNlNewMin = sci[S_HNLNEWMIN];
  s->hNlMinCtr = sci[S_HNLMINCTR];
  s->delayIdx = sci[S_DELAYIDX];
  s->stNearState = sci[S_STNEARSTATE];
  s->echoState = sci[S_ECHOSTATE];
  s->divergeState = sci[S_DIVERGESTATE];
  s->noiseEstCtr = sci[S_NOISEESTCTR];
  s->delayEstCtr = sci[S_DELAYESTCTR];
  s->seed = reinterpret_cast<const uint32_t*>(sc)[S_SEED];
}

// the far-end pre-buffer and the near / out rings of both bands: device-only data between kOffPre and the rows
// (dBufH, in their middle, belongs to AspAecState)
void keep_rings(float* blk, const float* cur) {
  memcpy(blk + kOffPre, cur + kOffPre, (kOffDBufH - kOffPre) * sizeof(float));
  memcpy(blk + kOffNearFrH, cur + kOffNearFrH, (kOffRows - kOffNearFrH) * sizeof(float));
}

void init_canonical(AspAecState* s) {  // WebRtcAec_InitAec float state, aec_core.c:1562-1610
  memset(s, 0, sizeof *s);
  for (int i = 0; i < 65; i++) s->dMinPow[i] = 1.0e6f;
  for (int i = 0; i < 65; i++) s->sd[i] = 1;
  for (int i = 0; i < 65; i++) s->sx[i] = 1;
  s->hNlFbMin = 1;
  s->hNlFbLocalMin = 1;
  s->hNlXdAvgMin = 1;
  s->overDrive = 2;
  s->overDriveSm = 2;
  s->seed = 777;
}

int check_running(AspAecBatch* b, const void* p, int n) {
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (p == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  if (n != 80 && n != 160) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  return 0;
}

// ------------------------------------------------------------------ per-stream control
// The reference takes the reported delay, Init and the call pattern per handle (echo_cancellation.c:341-347, 196-276).
// Once a caller uses AspAecBatch_ProcessV / _InitStream the batch keeps one AecCtl per stream (`per`); every call
// then runs the control functions once per stream -- on that stream's AecCtl, with a kStream issuer that records what
// they issue as that stream's descriptor; one far-end launch and one Process launch per call read the descriptors
// from device memory (aec_farend_v_kernel, aec_process_v_kernel).  A control-only handle keeps the AecCtl's alone.
int enter_vmode(AspAecBatch* b) {
  if (vmode(b)) return 0;
  if (b->su.num_high > 0 || b->su.delay_logging || !b->su.reported_delay_enabled || b->su.skewMode == kAecTrue || b->su.metricsMode)
    return aec_fail(ASP_ERR_STATE, "per-stream control covers the one-band configuration with reported delays "
                                   "(no delay logging / delay-agnostic mode / skew compensation / metrics)");
  DeviceIssuer iss(b, DeviceIssuer::kLaunch);
  if (const int rc = flush_pending_farend(b->su, iss)) return rc;
  if (!control_only(b) && !b->vproc_host) {
    AEC_TRY(hipHostMalloc((void**)&b->vproc_host, sizeof(AecStreamStep) * (size_t)b->S, hipHostMallocDefault));
    AEC_TRY(hipMalloc((void**)&b->vproc_dev, sizeof(AecStreamStep) * (size_t)b->S));
    AEC_TRY(hipHostMalloc((void**)&b->vfar_host, sizeof(FarOps) * (size_t)b->S, hipHostMallocDefault));
    AEC_TRY(hipMalloc((void**)&b->vfar_dev, sizeof(FarOps) * (size_t)b->S));
    AEC_TRY(hipEventCreateWithFlags(&b->vev, hipEventDisableTiming));
  }
  b->per.assign((size_t)b->S, b->ctl);
  return 0;
}

// WebRtcAec_BufferFarend of every stream, each on its own control plane
int buffer_farend_v(AspAecBatch* b, const float* far_dev, int n) {
  const bool dev = !control_only(b);
  if (dev) AEC_TRY(hipEventSynchronize(b->vev));  // the previous launches have read their descriptors
  for (int s = 0; s < b->S; ++s) {
    if (dev) memset(&b->vfar_host[s], 0, sizeof(FarOps));
    DeviceIssuer iss(b, DeviceIssuer::kStream, s);
    if (const int err = buffer_farend_device(b->su, b->per[(size_t)s], iss, far_dev, n)) return err;
  }
  if (!dev) return 0;
  AEC_TRY(hipMemcpyAsync(b->vfar_dev, b->vfar_host, sizeof(FarOps) * (size_t)b->S, hipMemcpyHostToDevice, b->stream));
  AEC_TRY(launch_aec_farend_v(b->state, b->far_ring, b->tables, far_dev, b->S, b->vfar_dev, n, b->su.num_part, b->stream));
  AEC_TRY(hipEventRecord(b->vev, b->stream));
  return 0;
}

// WebRtcAec_Process of every stream with its own reported delay; status[s] (may be null) receives the reference's
// return value of stream s (0, or -1 with lastError set: a delay outside 0 .. 500 ms still processes)
int process_v(AspAecBatch* b, const float* near_dev, float* out_dev, int n, const int16_t* ms, int ms_stride,
              int32_t* status, int* any_rc) {
  const bool dev = !control_only(b);
  if (dev) AEC_TRY(hipEventSynchronize(b->vev));
  *any_rc = 0;
  for (int s = 0; s < b->S; ++s) {
    if (dev) b->vproc_host[s].mode = 0;
    DeviceIssuer iss(b, DeviceIssuer::kStream, s);
    int rc = 0;
    if (const int err = process_device(b->su, b->per[(size_t)s], iss, n, ms[(size_t)s * ms_stride], &rc)) return err;
    if (status) status[s] = rc;
    *any_rc |= rc;
  }
  if (!dev) return 0;
  AEC_TRY(hipMemcpyAsync(b->vproc_dev, b->vproc_host, sizeof(AecStreamStep) * (size_t)b->S, hipMemcpyHostToDevice, b->stream));
  AEC_TRY(launch_aec_process_v(b->state, b->far_ring, b->tables, near_dev, out_dev, b->S, n, b->vproc_dev, b->su.num_part,
                               b->stream));
  AEC_TRY(hipEventRecord(b->vev, b->stream));
  return 0;
}
// ... and with one delay for all of them (the uniform-argument entry points on a batch under per-stream control)
int process_v(AspAecBatch* b, const float* near_dev, float* out_dev, int n, int msInSndCardBuf, int* rc) {
  const int16_t ms16 = (int16_t)(msInSndCardBuf < -32768 ? -32768 : msInSndCardBuf > 32767 ? 32767 : msInSndCardBuf);
  return process_v(b, near_dev, out_dev, n, &ms16, 0, nullptr, rc);
}

// BufferFarend + Process of one frame on device buffers (Run / TimedSteps): the batch's one control plane with the
// far-end work deferred into the Process launch, or every stream's own
int frame_device(AspAecBatch* b, DeviceIssuer& iss, const float* far_dev, const float* near_dev, float* out_dev, int n,
                 int msInSndCardBuf, int* rc) {
  if (vmode(b)) {
    if (const int err = buffer_farend_v(b, far_dev, n)) return err;
    return process_v(b, near_dev, out_dev, n, msInSndCardBuf, rc);
  }
  iss.near = near_dev;
  iss.out = out_dev;
  if (const int err = buffer_farend_device(b->su, b->ctl, iss, far_dev, n, true)) return err;
  return process_device(b->su, b->ctl, iss, n, msInSndCardBuf, rc);
}

// ------------------------------------------------------------------ list calls (AspAecBatch_RunList)
static_assert(kAecListMaxFrames == ASP_AEC_LIST_MAX_FRAMES && kAecListSlots == ASP_AEC_LIST_SLOTS && sizeof(AecListStep) == 176 &&
                  sizeof(AecListEntry) == 8, "the figures include/asp_aec.h states");
size_t list_slot_bytes(const AspAecBatch* b) {
  return (size_t)b->S * (sizeof(AecListEntry) + (size_t)kAecListMaxFrames * sizeof(AecListStep));
}
int list_resources(AspAecBatch* b) {
  if (b->list_dev) return 0;
  AEC_TRY(hipHostMalloc((void**)&b->list_host, list_slot_bytes(b) * kAecListSlots, hipHostMallocDefault));
  for (int i = 0; i < kAecListSlots; ++i) AEC_TRY(hipEventCreateWithFlags(&b->list_ev[i], hipEventDisableTiming));
  AEC_TRY(hipMalloc((void**)&b->list_dev, list_slot_bytes(b) * kAecListSlots));
  b->list_slot = 0;
  return 0;
}
// the descriptors of one launch: [entry][frame] with `stride` frames per entry, or nowhere (a control-only handle)
struct ListSlotSink final : AecListSink {
  AecListStep* descs = nullptr;
  int stride = 0;
  int step(int entry, int frame, const AecListStep& d) override {
    if (descs) descs[(size_t)entry * stride + frame] = d;
    return 0;
  }
};

}  // namespace

extern "C" {

int AspAecBatch_Create(AspAecBatch** out, int num_streams, int device) {
  AspDeviceScope dev_scope_;
  if (!out || num_streams <= 0) return aec_fail(ASP_ERR_PARAM, "AspAecBatch_Create: bad argument");
  *out = nullptr;
  if (int rc = dev_scope_.select("asp_aec", device, ASP_ERR_PARAM, "no HIP device: the echo canceller has no CPU fallback")) return rc;
  AspAecBatch* b = new AspAecBatch();
  b->S = num_streams;
  b->device = device;
  hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  b->own_stream = e == hipSuccess;
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, state_bytes(b));
  if (e == hipSuccess) e = hipMalloc((void**)&b->far_ring, far_bytes(b));
  if (e == hipSuccess) e = hipMalloc((void**)&b->tables, sizeof(AecTables));
  if (e == hipSuccess) e = hipMalloc((void**)&b->stage_far, (size_t)num_streams * 160 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->stage_near, (size_t)num_streams * 160 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->stage_out, (size_t)num_streams * 160 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->stage_near_h, (size_t)num_streams * 160 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->stage_out_h, (size_t)num_streams * 160 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->metrics, (size_t)num_streams * kMetDwords * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->rs_buffer, (size_t)num_streams * kResamplerBufferSize * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->stage_rs, (size_t)num_streams * kResamplerBufferSize * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->dblocks, (size_t)num_streams * sizeof(DelayBlock));
  if (e == hipSuccess) e = hipMalloc((void**)&b->spectra, (size_t)num_streams * kSpecBlocks * kSpecDwords * sizeof(float));
  if (e == hipSuccess) {  // WebRtc_set_lookahead at Create (aec_core.c:1374-1378); the Init functions leave it alone
    std::vector<DelayBlock> all((size_t)num_streams);
    memset(all.data(), 0, all.size() * sizeof(DelayBlock));
    for (auto& d : all) d.s.lookahead = ASP_AEC_DELAY_LOOKAHEAD;
    e = hipMemcpy(b->dblocks, all.data(), all.size() * sizeof(DelayBlock), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipEventCreate(&b->ev0);
  if (e == hipSuccess) e = hipEventCreate(&b->ev1);
  if (e == hipSuccess) {
    AecTables T;
    build_tables(&T);
    e = hipMemcpy(b->tables, &T, sizeof T, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    AspAecBatch_Free(b);
    return aec_fail(ASP_ERR_HIP, "AspAecBatch_Create", e);
  }
  *out = b;
  return ASP_OK;
}

// The integer control plane alone (no device is touched, nothing is launched): BufferFarend /
// Process / set_config / GetControl behave as on a real batch, so the host logic can be checked
// against the oracle on a machine without a GPU.  Every data-touching entry point refuses it.
int AspAecBatch_CreateControlOnly(AspAecBatch** out, int num_streams) {
  AspDeviceScope dev_scope_;
  if (!out || num_streams <= 0) return aec_fail(ASP_ERR_PARAM, "AspAecBatch_CreateControlOnly: bad argument");
  AspAecBatch* b = new AspAecBatch();
  b->S = num_streams;
  b->device = -1;
  *out = b;
  return ASP_OK;
}

int AspAecBatch_Free(AspAecBatch* b) {
  AspDeviceScope dev_scope_;
  if (!b) return -1;
  if (control_only(b)) {
    delete b;
    return 0;
  }
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->state) (void)hipFree(b->state);
  if (b->far_ring) (void)hipFree(b->far_ring);
  if (b->tables) (void)hipFree(b->tables);
  if (b->stage_far) (void)hipFree(b->stage_far);
  if (b->stage_near) (void)hipFree(b->stage_near);
  if (b->stage_out) (void)hipFree(b->stage_out);
  if (b->stage_near_h) (void)hipFree(b->stage_near_h);
  if (b->stage_out_h) (void)hipFree(b->stage_out_h);
  if (b->metrics) (void)hipFree(b->metrics);
  if (b->dblocks) (void)hipFree(b->dblocks);
  if (b->rs_buffer) (void)hipFree(b->rs_buffer);
  if (b->stage_rs) (void)hipFree(b->stage_rs);
  if (b->spectra) (void)hipFree(b->spectra);
  if (b->vproc_host) (void)hipHostFree(b->vproc_host);
  if (b->vproc_dev) (void)hipFree(b->vproc_dev);
  if (b->vfar_host) (void)hipHostFree(b->vfar_host);
  if (b->vfar_dev) (void)hipFree(b->vfar_dev);
  if (b->vev) (void)hipEventDestroy(b->vev);
  if (b->list_host) (void)hipHostFree(b->list_host);
  if (b->list_dev) (void)hipFree(b->list_dev);
  for (int i = 0; i < kAecListSlots; ++i)
    if (b->list_ev[i]) (void)hipEventDestroy(b->list_ev[i]);
  b->sync.release();
  if (b->flow_bits) (void)hipFree(b->flow_bits);
  if (b->flow_dev) (void)hipFree(b->flow_dev);
  if (b->flow_host) (void)hipHostFree(b->flow_host);
  for (int i = 0; i < 4; ++i)
    if (b->flow_ev[i]) (void)hipEventDestroy(b->flow_ev[i]);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->side) {
    (void)hipStreamSynchronize(b->side);
    (void)hipStreamDestroy(b->side);
    (void)hipEventDestroy(b->ev_fork);
    (void)hipEventDestroy(b->ev_join);
  }
  if (b->stream && b->own_stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return 0;
}

int AspAecBatch_num_streams(const AspAecBatch* b) { return b ? b->S : 0; }
int AspAecBatch_get_error_code(const AspAecBatch* b) { return b ? ctl_of(b, 0).lastError : AEC_NULL_POINTER_ERROR; }

int AspAecBatch_set_config(AspAecBatch* b, AecConfig config) {  // echo_cancellation.c:410-438
  AspDeviceScope dev_scope_;
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  if (config.skewMode != kAecFalse && config.skewMode != kAecTrue) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  b->su.skewMode = config.skewMode;
  if (config.nlpMode != kAecNlpConservative && config.nlpMode != kAecNlpModerate &&
      config.nlpMode != kAecNlpAggressive) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  if (config.metricsMode != kAecFalse && config.metricsMode != kAecTrue) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  if (config.delay_logging != kAecFalse && config.delay_logging != kAecTrue) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  // per-stream control: the suppression level (the batch's, as every mode); the optional modes are not covered
  if (vmode(b) && (config.skewMode == kAecTrue || config.metricsMode == kAecTrue || config.delay_logging == kAecTrue))
    return aec_fail(ASP_ERR_STATE, "set_config: per-stream control covers nlpMode only; Init the batch to switch modes");
  b->su.nlp_mode = config.nlpMode;  // WebRtcAec_SetConfigCore, aec_core.c:1844-1862
  b->su.metricsMode = config.metricsMode;
  if (b->su.metricsMode && !control_only(b)) {
    const int err = init_metrics_device(b, dev_scope_);
    if (err) return err;
  }
  b->su.delay_logging = config.delay_logging;
  if (b->su.delay_logging && !control_only(b)) {  // memset(delay_histogram), aec_core.c:1858-1860
    AEC_TRY(dev_scope_.select(b->device));
    AEC_TRY(hipMemset2DAsync(reinterpret_cast<char*>(b->dblocks) + offsetof(DelayBlock, s.delay_histogram), sizeof(DelayBlock), 0,
                             sizeof(((AspAecDelayState*)nullptr)->delay_histogram), (size_t)b->S, b->stream));
  }
  return 0;
}

int AspAecBatch_Init(AspAecBatch* b, int32_t sampFreq, int32_t scSampFreq) {  // echo_cancellation.c:196-276
  AspDeviceScope dev_scope_;
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (sampFreq != 8000 && sampFreq != 16000 && sampFreq != 32000 && sampFreq != 48000) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  // 48 kHz: the reference's own mult breaks there (aec_core.c:1541-1543)
  if (sampFreq > 32000) return set_error(b, AEC_UNSUPPORTED_FUNCTION_ERROR);
  b->su.sampFreq = sampFreq;
  if (scSampFreq < 1 || scSampFreq > 96000) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  b->ctl.lastError = ctl0(b).lastError;  // (Init does not clear the error code)
  b->per.clear();                        // back to one control plane for the batch
  const int old_num_part = b->su.num_part;
  init_control(b->su, b->ctl, sampFreq, scSampFreq);
  if (!control_only(b)) {
    AEC_TRY(dev_scope_.select(b->device));
    AEC_TRY(hipStreamSynchronize(b->stream));
    if (old_num_part != kNumPartNormal) {  // back to the 12-partition blocks
      AEC_TRY(hipFree(b->state));
      b->state = nullptr;
      AEC_TRY(hipMalloc((void**)&b->state, state_bytes(b)));
    }
    const int kStateDwords = state_dwords(b);
    std::vector<AspAecState> s0(1);  // ~50 KB, per call: two batches may be initialised from two host threads at once
    init_canonical(s0.data());
    std::vector<float> blk(kStateDwords);
    pack_stream(b->su.num_part, b->ctl, s0.data(), blk.data());
    std::vector<float> all((size_t)b->S * kStateDwords);
    for (int s = 0; s < b->S; ++s) memcpy(all.data() + (size_t)s * kStateDwords, blk.data(), kStateDwords * sizeof(float));
    AEC_TRY(hipMemcpy(b->state, all.data(), state_bytes(b), hipMemcpyHostToDevice));
    // on the batch's own (non-blocking) stream: a null-stream memset is not ordered with its kernels
    AEC_TRY(hipMemsetAsync(b->far_ring, 0, far_bytes(b), b->stream));  // WebRtc_InitBuffer zeroes the rings
    AEC_TRY(hipStreamSynchronize(b->stream));
    const int err = init_metrics_device(b, dev_scope_);  // aec_core.c:1612-1613
    if (err) return err;
    const int err2 = init_delay_device(b, dev_scope_);   // aec_core.c:1502-1516
    if (err2) return err2;
    // WebRtcAec_InitResampler (echo_cancellation.c:221, aec_resampler.c:55-66)
    AEC_TRY(hipMemsetAsync(b->rs_buffer, 0, (size_t)b->S * kResamplerBufferSize * sizeof(float), b->stream));
  }
  return 0;
}

int AspAecBatch_BufferFarend(AspAecBatch* b, const float* farend, int nrOfSamples, int mem) {
  AspDeviceScope dev_scope_;
  const int chk = check_running(b, farend, nrOfSamples);
  if (chk != 0) return chk;
  const bool staged = mem == ASP_MEM_HOST && !control_only(b);
  if (!control_only(b)) AEC_TRY(dev_scope_.select(b->device));
  const float* dev = farend;
  if (staged) {
    AEC_TRY(hipMemcpyAsync(b->stage_far, farend, (size_t)b->S * nrOfSamples * sizeof(float), hipMemcpyHostToDevice, b->stream));
    dev = b->stage_far;
  }
  DeviceIssuer iss(b, DeviceIssuer::kLaunch);
  const int rc = vmode(b) ? buffer_farend_v(b, dev, nrOfSamples) : buffer_farend_device(b->su, b->ctl, iss, dev, nrOfSamples);
  if (rc != 0) return rc;
  if (staged) AEC_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

static int process_impl(AspAecBatch* b, AspDeviceScope& dev_scope_, const float* nearend, const float* near_high, float* out,
                        float* out_high, int nrOfSamples, int msInSndCardBuf, int mem, int32_t skew);

int AspAecBatch_Process(AspAecBatch* b, const float* nearend, float* out, int nrOfSamples,
                        int msInSndCardBuf, int32_t skew, int mem) {
  AspDeviceScope dev_scope_;
  if (b && b->su.num_high > 0) return set_error(b, AEC_BAD_PARAMETER_ERROR);  // a 32 kHz batch needs both bands (ProcessBands)
  return process_impl(b, dev_scope_, nearend, nullptr, out, nullptr, nrOfSamples, msInSndCardBuf, mem, skew);
}

int AspAecBatch_ProcessBands(AspAecBatch* b, const float* near_low, const float* near_high,
                             float* out_low, float* out_high, int nrOfSamples, int msInSndCardBuf,
                             int32_t skew, int mem) {
  AspDeviceScope dev_scope_;
  if (b && (b->su.num_high < 1 || near_high == nullptr || out_high == nullptr))
    return set_error(b, b->su.num_high < 1 ? AEC_BAD_PARAMETER_ERROR : AEC_NULL_POINTER_ERROR);
  return process_impl(b, dev_scope_, near_low, near_high, out_low, out_high, nrOfSamples, msInSndCardBuf, mem, skew);
}

int AspAecBatch_num_bands(const AspAecBatch* b) { return b ? 1 + b->su.num_high : 0; }

// WebRtcAec_Process of every stream with the stream's OWN reported delay (echo_cancellation.c:341-347 takes it per
// handle): msInSndCardBuf[num_streams]; skew[num_streams] may be null (skew compensation is not covered by the
// per-stream control); status[num_streams] (may be null) receives each stream's reference return value.
int AspAecBatch_ProcessV(AspAecBatch* b, const float* nearend, float* out, int nrOfSamples, const int16_t* msInSndCardBuf,
                         const int32_t* skew, int32_t* status, int mem) {
  AspDeviceScope dev_scope_;
  (void)skew;
  if (b && out == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  const int chk = check_running(b, nearend, nrOfSamples);
  if (chk != 0) return chk;
  if (!msInSndCardBuf) return aec_fail(ASP_ERR_PARAM, "ProcessV: null delay array");
  if (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE) return aec_fail(ASP_ERR_PARAM, "mem must be ASP_MEM_HOST or ASP_MEM_DEVICE");
  const bool staged = mem == ASP_MEM_HOST && !control_only(b);
  if (!control_only(b)) AEC_TRY(dev_scope_.select(b->device));
  if (const int rc = enter_vmode(b)) return rc;
  const size_t bytes = (size_t)b->S * nrOfSamples * sizeof(float);
  const float* nd = nearend;
  float* od = out;
  if (staged) {
    AEC_TRY(hipMemcpyAsync(b->stage_near, nearend, bytes, hipMemcpyHostToDevice, b->stream));
    nd = b->stage_near;
    od = b->stage_out;
  }
  int rc = 0;
  const int err = process_v(b, nd, od, nrOfSamples, msInSndCardBuf, 1, status, &rc);
  if (err != 0) return err;
  if (staged) {
    AEC_TRY(hipMemcpyAsync(out, od, bytes, hipMemcpyDeviceToHost, b->stream));
    AEC_TRY(hipStreamSynchronize(b->stream));
  }
  return rc;
}

// WebRtcAec_Init of ONE stream of a running batch (echo_cancellation.c:196-276 per handle): its control plane, its
// state block and its far-ring slots go back to their initial values at the batch's sample rates; the other streams
// are untouched.  The filter length (AspAecBatch_enable_delay_correction) stays the batch's.
int AspAecBatch_InitStream(AspAecBatch* b, int stream) {
  AspDeviceScope dev_scope_;
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  if (stream < 0 || stream >= b->S) return aec_fail(ASP_ERR_PARAM, "InitStream: stream out of range");
  if (!control_only(b)) AEC_TRY(dev_scope_.select(b->device));
  if (const int rc = enter_vmode(b)) return rc;
  // the stream's share of Init; the setup -- filter length, suppression level, rates -- stays the batch's
  if (!control_only(b)) AEC_TRY(hipStreamSynchronize(b->stream));
  init_stream_control(b->per[(size_t)stream]);
  if (control_only(b)) return 0;
  const int kStateDwords = state_dwords(b);
  std::vector<AspAecState> s0(1);
  init_canonical(s0.data());
  std::vector<float> blk(kStateDwords);
  pack_stream(b->su.num_part, b->per[(size_t)stream], s0.data(), blk.data());
  AEC_TRY(hipMemcpy(b->state + (size_t)stream * kStateDwords, blk.data(), (size_t)kStateDwords * sizeof(float), hipMemcpyHostToDevice));
  // WebRtc_InitBuffer zeroes the far rings: the stream's slice of every slot
  AEC_TRY(hipMemset2D(b->far_ring + (size_t)stream * kFarSlotDwords, (size_t)b->S * kFarSlotDwords * sizeof(float), 0,
                      (size_t)kFarSlotDwords * sizeof(float), (size_t)kFarSlots));
  return 0;
}

static void fill_control(const AecCtl& k, AspAecControl* c);

int AspAecBatch_GetControlStream(AspAecBatch* b, int stream, AspAecControl* c) {
  if (!b || !c || stream < 0 || stream >= b->S) return aec_fail(ASP_ERR_PARAM, "GetControlStream: bad argument");
  fill_control(ctl_of(b, stream), c);
  return ASP_OK;
}

// WebRtcAec_BufferFarend + WebRtcAec_Process of SOME streams, each by its own number of frames (include/asp_aec.h).
// Everything is checked first; the control functions then run on copies of the listed streams' control planes, one
// launch's frames at a time (aec_control.h, plan_list), and a launch's copies are committed once it is enqueued.
int AspAecBatch_RunList(AspAecBatch* b, const int32_t* streams, const int32_t* counts, int n, const float* farend,
                        const float* nearend, float* out, int nrOfSamples, int max_frames, const int16_t* msInSndCardBuf,
                        int32_t* status, int mem) {
  AspDeviceScope dev_scope_;
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (!streams || !counts || !farend || !nearend || !out || !msInSndCardBuf)
    return aec_fail(ASP_ERR_PARAM, "RunList: null pointer (only status may be null)");
  if (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE) return aec_fail(ASP_ERR_PARAM, "mem must be ASP_MEM_HOST or ASP_MEM_DEVICE");
  if (nrOfSamples != 80 && nrOfSamples != 160) return aec_fail(ASP_ERR_PARAM, "RunList: nrOfSamples must be 80 or 160");
  if (n < 0 || n > b->S) return aec_fail(ASP_ERR_PARAM, "RunList: n outside 0 .. num_streams");
  if (max_frames < 0) return aec_fail(ASP_ERR_PARAM, "RunList: max_frames < 0");
  int maxc = 0;
  {
    std::vector<char> seen((size_t)b->S, 0);
    for (int i = 0; i < n; ++i) {
      if (streams[i] < 0 || streams[i] >= b->S) return aec_fail(ASP_ERR_PARAM, "RunList: stream outside the batch");
      if (seen[(size_t)streams[i]]) return aec_fail(ASP_ERR_PARAM, "RunList: stream listed twice");
      seen[(size_t)streams[i]] = 1;
      if (counts[i] < 0 || counts[i] > max_frames) return aec_fail(ASP_ERR_PARAM, "RunList: count outside 0 .. max_frames");
      if (counts[i] > maxc) maxc = counts[i];
    }
  }
  if (b->su.initFlag != kInitCheck) return aec_fail(ASP_ERR_STATE, "RunList: the batch is not initialised");
  if (b->su.num_high > 0 || b->su.delay_logging || !b->su.reported_delay_enabled || b->su.skewMode == kAecTrue || b->su.metricsMode)
    return aec_fail(ASP_ERR_STATE, "per-stream control covers the one-band configuration with reported delays "
                                   "(no delay logging / delay-agnostic mode / skew compensation / metrics)");
  if (n == 0 || max_frames == 0) return ASP_OK;  // nothing to do: the batch stays as it is, mode included
  const bool dev = !control_only(b);
  if (dev) AEC_TRY(dev_scope_.select(b->device));
  if (const int rc = enter_vmode(b)) return rc;
  if (maxc == 0) return ASP_OK;
  if (dev) {
    if (const int rc = list_resources(b)) return rc;
  }
  std::vector<AecCtl> work((size_t)n);
  for (int i = 0; i < n; ++i) work[(size_t)i] = b->per[(size_t)streams[i]];
  std::vector<int32_t> rcs((size_t)n, 0);
  auto commit = [&] {
    for (int i = 0; i < n; ++i) b->per[(size_t)streams[i]] = work[(size_t)i];
  };
  auto finish = [&] {
    int any = 0;
    for (int i = 0; i < n; ++i) {
      if (status) status[i] = rcs[(size_t)i];
      any |= rcs[(size_t)i];
    }
    return any;
  };
  ListSlotSink sink;
  if (!dev) {
    if (const int err = plan_list(b->su, work.data(), counts, n, 0, maxc, nrOfSamples, msInSndCardBuf, rcs.data(), sink)) return err;
    commit();
    return finish();
  }
  const size_t row = (size_t)n * nrOfSamples;  // one frame of all entries
  const int chunk = maxc < kAecListMaxFrames ? maxc : kAecListMaxFrames;
  const bool staged = mem == ASP_MEM_HOST;
  float *dfar = nullptr, *dnear = nullptr, *dout = nullptr;
  std::vector<float> back;
  if (staged) {
    hipError_t e = hipMalloc((void**)&dfar, row * chunk * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dnear, row * chunk * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, row * chunk * sizeof(float));
    if (e != hipSuccess) {
      if (dfar) (void)hipFree(dfar);
      if (dnear) (void)hipFree(dnear);
      return aec_fail(ASP_ERR_HIP, "RunList: staging", e);
    }
    back.resize(row * chunk);
  }
  int err = 0;
  auto hip_step = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && err == 0) err = aec_fail(ASP_ERR_HIP, what, e);
    return err == 0;
  };
  for (int f0 = 0; f0 < maxc && err == 0; f0 += kAecListMaxFrames) {
    const int nf = maxc - f0 < kAecListMaxFrames ? maxc - f0 : kAecListMaxFrames;
    const int slot = b->list_slot;
    // the slot's previous launch must have read its descriptors before they are overwritten (a full ring: wait here)
    if (!hip_step(hipEventSynchronize(b->list_ev[slot]), "RunList: descriptor slot")) break;
    unsigned char* h = b->list_host + (size_t)slot * list_slot_bytes(b);
    unsigned char* d = b->list_dev + (size_t)slot * list_slot_bytes(b);
    AecListEntry* entries = reinterpret_cast<AecListEntry*>(h);
    for (int i = 0; i < n; ++i) {
      const int left = counts[i] - f0;
      entries[i].stream = streams[i];
      entries[i].count = left < 0 ? 0 : left < nf ? left : nf;
    }
    sink.descs = reinterpret_cast<AecListStep*>(h + (size_t)n * sizeof(AecListEntry));
    sink.stride = nf;
    err = plan_list(b->su, work.data(), counts, n, f0, nf, nrOfSamples, msInSndCardBuf, rcs.data(), sink);
    if (err != 0) break;
    const float *lf = farend + row * f0, *ln = nearend + row * f0;
    float* lo = out + row * f0;
    if (staged) {
      if (!hip_step(hipMemcpyAsync(dfar, lf, row * nf * sizeof(float), hipMemcpyHostToDevice, b->stream), "RunList: upload")) break;
      if (!hip_step(hipMemcpyAsync(dnear, ln, row * nf * sizeof(float), hipMemcpyHostToDevice, b->stream), "RunList: upload")) break;
      lf = dfar;
      ln = dnear;
      lo = dout;
    }
    const size_t bytes = (size_t)n * sizeof(AecListEntry) + (size_t)n * nf * sizeof(AecListStep);
    if (!hip_step(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, b->stream), "RunList: descriptors")) break;
    if (!hip_step(launch_aec_list(b->state, b->far_ring, b->tables, lf, ln, lo, b->S, nrOfSamples, n,
                                  reinterpret_cast<const AecListEntry*>(d),
                                  reinterpret_cast<const AecListStep*>(d + (size_t)n * sizeof(AecListEntry)), nf,
                                  batch_proc_ops(b->su), b->su.num_part, b->stream), "RunList: launch")) break;
    commit();  // the device is now ahead by this launch's frames whatever follows
    if (!hip_step(hipEventRecord(b->list_ev[slot], b->stream), "RunList: descriptor slot")) break;
    b->list_slot = (slot + 1) % kAecListSlots;
    if (staged) {
      // only the rows the launch wrote go back: rows f >= counts[i] of `out` stay the caller's
      if (!hip_step(hipMemcpyAsync(back.data(), dout, row * nf * sizeof(float), hipMemcpyDeviceToHost, b->stream), "RunList: download")) break;
      if (!hip_step(hipStreamSynchronize(b->stream), "RunList: download")) break;
      for (int i = 0; i < n; ++i)
        for (int f = 0; f < entries[i].count; ++f)
          memcpy(out + row * (f0 + f) + (size_t)i * nrOfSamples, back.data() + row * f + (size_t)i * nrOfSamples,
                 (size_t)nrOfSamples * sizeof(float));
    }
  }
  if (staged) {
    (void)hipStreamSynchronize(b->stream);
    (void)hipFree(dfar);
    (void)hipFree(dnear);
    (void)hipFree(dout);
  }
  if (err != 0) return err;
  return finish();
}

static int process_impl(AspAecBatch* b, AspDeviceScope& dev_scope_, const float* nearend, const float* near_high, float* out,
                        float* out_high, int nrOfSamples, int msInSndCardBuf, int mem, int32_t skew) {
  if (b && out == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  const int chk = check_running(b, nearend, nrOfSamples);
  if (chk != 0) return chk;
  const bool staged = mem == ASP_MEM_HOST && !control_only(b);
  if (!control_only(b)) AEC_TRY(dev_scope_.select(b->device));
  const size_t bytes = (size_t)b->S * nrOfSamples * sizeof(float);
  DeviceIssuer iss(b, DeviceIssuer::kLaunch);
  iss.near = nearend;
  iss.out = out;
  iss.near_high = near_high;
  iss.out_high = out_high;
  if (staged) {
    AEC_TRY(hipMemcpyAsync(b->stage_near, nearend, bytes, hipMemcpyHostToDevice, b->stream));
    iss.near = b->stage_near;
    iss.out = b->stage_out;
    if (b->su.num_high > 0) {
      AEC_TRY(hipMemcpyAsync(b->stage_near_h, near_high, bytes, hipMemcpyHostToDevice, b->stream));
      iss.near_high = b->stage_near_h;
      iss.out_high = b->stage_out_h;
    }
  }
  int rc = 0;
  // (with per-stream control: the same delay for every stream's own control plane)
  const int err = vmode(b) ? process_v(b, iss.near, iss.out, nrOfSamples, msInSndCardBuf, &rc)
                           : process_device(b->su, b->ctl, iss, nrOfSamples, msInSndCardBuf, &rc, skew);
  if (err != 0) return err;
  if (staged) {
    AEC_TRY(hipMemcpyAsync(out, iss.out, bytes, hipMemcpyDeviceToHost, b->stream));
    if (b->su.num_high > 0)
      AEC_TRY(hipMemcpyAsync(out_high, b->stage_out_h, bytes, hipMemcpyDeviceToHost, b->stream));
    AEC_TRY(hipStreamSynchronize(b->stream));
  }
  return rc;
}

int AspAecBatch_Run(AspAecBatch* b, const float* farend, const float* nearend, float* out,
                    int nrOfSamples, int num_frames, int msInSndCardBuf, int mem) {
  AspDeviceScope dev_scope_;
  if (b && b->su.num_high > 0) return aec_fail(ASP_ERR_STATE, "AspAecBatch_Run: single-band batches only (use ProcessBands)");
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_Run: control-only handle");
  if (b && out == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  int chk = check_running(b, farend, nrOfSamples);
  if (chk == 0) chk = check_running(b, nearend, nrOfSamples);
  if (chk != 0) return chk;
  if (num_frames < 0) return aec_fail(ASP_ERR_PARAM, "Run: num_frames < 0");
  if (b->su.skewMode == kAecTrue)  // the skew estimate is a function of the calls' skew arguments: Process / ProcessBands carry one
    return aec_fail(ASP_ERR_STATE, "Run: no skew argument; with skew compensation on, feed the frames through BufferFarend / Process");
  AEC_TRY(dev_scope_.select(b->device));
  const size_t per = (size_t)b->S * nrOfSamples;
  int rc_all = 0;
  if (mem == ASP_MEM_HOST) {
    // stream the frames through device staging in chunks of up to 64 frames
    const int chunk = 64;
    float *dfar = nullptr, *dnear = nullptr, *dout = nullptr;
    AEC_TRY(hipMalloc((void**)&dfar, per * chunk * sizeof(float)));
    hipError_t e = hipMalloc((void**)&dnear, per * chunk * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&dout, per * chunk * sizeof(float));
    int err = e == hipSuccess ? 0 : aec_fail(ASP_ERR_HIP, "Run: staging", e);
    for (int f0 = 0; err == 0 && f0 < num_frames; f0 += chunk) {
      const int nf = num_frames - f0 < chunk ? num_frames - f0 : chunk;
      e = hipMemcpyAsync(dfar, farend + per * f0, per * nf * sizeof(float), hipMemcpyHostToDevice, b->stream);
      if (e == hipSuccess)
        e = hipMemcpyAsync(dnear, nearend + per * f0, per * nf * sizeof(float), hipMemcpyHostToDevice, b->stream);
      if (e != hipSuccess) {
        err = aec_fail(ASP_ERR_HIP, "Run: upload", e);
        break;
      }
      DeviceIssuer iss(b, aec_flow_applies(b, nf) && aec_flow_resources(b) == 0 ? DeviceIssuer::kHandoff : DeviceIssuer::kLaunch);
      for (int f = 0; f < nf && err == 0; ++f) {
        int rc = 0;
        err = frame_device(b, iss, dfar + per * f, dnear + per * f, dout + per * f, nrOfSamples, msInSndCardBuf, &rc);
        rc_all |= rc;
      }
      if (err == 0) err = iss.finish();
      if (err == 0) {
        e = hipMemcpyAsync(out + per * f0, dout, per * nf * sizeof(float), hipMemcpyDeviceToHost, b->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
        if (e != hipSuccess) err = aec_fail(ASP_ERR_HIP, "Run: download", e);
      }
    }
    (void)hipStreamSynchronize(b->stream);
    if (err == 0) err = aec_flow_check(b);
    if (dfar) (void)hipFree(dfar);
    if (dnear) (void)hipFree(dnear);
    if (dout) (void)hipFree(dout);
    if (err != 0) return err;
    return rc_all;
  }
  const bool flow = aec_flow_applies(b, num_frames);
  if (flow) {
    if (const int rcf = aec_flow_resources(b)) return rcf;
  }
  DeviceIssuer iss(b, flow ? DeviceIssuer::kHandoff : DeviceIssuer::kLaunch);
  for (int f = 0; f < num_frames; ++f) {
    int rc = 0;
    if (const int err = frame_device(b, iss, farend + per * f, nearend + per * f, out + per * f, nrOfSamples, msInSndCardBuf, &rc))
      return err;
    rc_all |= rc;
  }
  if (const int rcf = iss.finish()) return rcf;
  return rc_all;
}

int AspAecBatch_TimedSteps(AspAecBatch* b, const float* farend, const float* nearend, float* out,
                           int nrOfSamples, int frames_in_ring, int steps, float* elapsed_ms) {
  AspDeviceScope dev_scope_;
  if (b && b->su.num_high > 0) return aec_fail(ASP_ERR_STATE, "AspAecBatch_TimedSteps: single-band batches only (use ProcessBands)");
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_TimedSteps: control-only handle");
  if (!b || !farend || !nearend || !out || frames_in_ring <= 0 || steps < 0 || !elapsed_ms)
    return aec_fail(ASP_ERR_PARAM, "TimedSteps: bad argument");
  if (check_running(b, farend, nrOfSamples) != 0) return -1;
  if (b->su.skewMode == kAecTrue)
    return aec_fail(ASP_ERR_STATE, "TimedSteps: no skew argument; with skew compensation on, feed the frames through BufferFarend / Process");
  AEC_TRY(dev_scope_.select(b->device));
  const size_t per = (size_t)b->S * nrOfSamples;
  // two chains when the batch is large enough to fill the chip twice over and past its start-up phase
  // (whose pass-through copies stay on the main stream); ASP_AEC_CHAINS=1 keeps one
  const char* ch = getenv("ASP_AEC_CHAINS");
  const bool flow = aec_flow_applies(b, steps);
  if (flow) {
    const int rcf = aec_flow_resources(b);
    if (rcf != 0) return rcf;
  }
  const bool dual = !flow && !vmode(b) && b->S >= 2048 && !b->ctl.startup_phase && !(ch && atoi(ch) == 1) &&
                    !b->su.delay_logging && b->su.reported_delay_enabled && !b->su.skewMode;
  if (dual && !b->side) {
    AEC_TRY(hipStreamCreateWithFlags(&b->side, hipStreamNonBlocking));
    AEC_TRY(hipEventCreateWithFlags(&b->ev_fork, hipEventDisableTiming));
    AEC_TRY(hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming));
  }
  AEC_TRY(hipEventRecord(b->ev0, b->stream));
  if (dual) {
    AEC_TRY(hipEventRecord(b->ev_fork, b->stream));
    AEC_TRY(hipStreamWaitEvent(b->side, b->ev_fork, 0));
  }
  int err = 0;
  DeviceIssuer iss(b, flow ? DeviceIssuer::kHandoff : DeviceIssuer::kLaunch);
  if (dual) iss.side = b->side;
  for (int k = 0; k < steps && err == 0; ++k) {
    const size_t off = per * (size_t)(k % frames_in_ring);
    int rc = 0;
    err = frame_device(b, iss, farend + off, nearend + off, out + off, nrOfSamples, 0, &rc);
  }
  if (err == 0) err = iss.finish();
  if (dual) {
    AEC_TRY(hipEventRecord(b->ev_join, b->side));
    AEC_TRY(hipStreamWaitEvent(b->stream, b->ev_join, 0));
  }
  if (err != 0) return err;
  AEC_TRY(hipEventRecord(b->ev1, b->stream));
  AEC_TRY(hipEventSynchronize(b->ev1));
  AEC_TRY(hipEventElapsedTime(elapsed_ms, b->ev0, b->ev1));
  return aec_flow_check(b);
}

int AspAecBatch_Synchronize(AspAecBatch* b) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_Synchronize: control-only handle");
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  return aec_flow_check(b);
}

void* AspAecBatch_GetStream(AspAecBatch* b) { return b && !control_only(b) ? (void*)b->stream : nullptr; }

int AspAecBatch_SetFlow(AspAecBatch* b, int mode) {
  AspDeviceScope dev_scope_;
  if (!b || mode < -1 || mode > 1) return aec_fail(ASP_ERR_PARAM, "SetFlow: -1 (default), 0 (off) or 1 (on)");
  b->flow = mode;
  return ASP_OK;
}

int AspAecBatch_ExportState(AspAecBatch* b, int stream, AspAecState* out) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_ExportState: control-only handle");
  if (!b || !out || stream < 0 || stream >= b->S) return aec_fail(ASP_ERR_PARAM, "ExportState: bad argument");
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  const int kStateDwords = state_dwords(b);
  std::vector<float> blk(kStateDwords);
  AEC_TRY(hipMemcpy(blk.data(), b->state + (size_t)stream * kStateDwords, kStateDwords * sizeof(float), hipMemcpyDeviceToHost));
  unpack_stream(b->su.num_part, ctl_of(b, stream), blk.data(), out);  // the partition positions of the block are the stream's own
  return ASP_OK;
}

int AspAecBatch_ImportState(AspAecBatch* b, int stream, const AspAecState* in) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_ImportState: control-only handle");
  if (!b || !in || stream < 0 || stream >= b->S) return aec_fail(ASP_ERR_PARAM, "ImportState: bad argument");
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  const int kStateDwords = state_dwords(b);
  std::vector<float> blk(kStateDwords), cur(kStateDwords);
  AEC_TRY(hipMemcpy(cur.data(), b->state + (size_t)stream * kStateDwords, kStateDwords * sizeof(float), hipMemcpyDeviceToHost));
  pack_stream(b->su.num_part, ctl_of(b, stream), in, blk.data());
  // the time-domain rings are not part of AspAecState: keep the stream's own
  keep_rings(blk.data(), cur.data());
  AEC_TRY(hipMemcpy(b->state + (size_t)stream * kStateDwords, blk.data(), kStateDwords * sizeof(float), hipMemcpyHostToDevice));
  return ASP_OK;
}

// WebRtcAec_enable_delay_correction(WebRtcAec_aec_core(inst), enable) for every stream of the batch
// (aec_core.c:1876-1881): 32 partitions and the extended constants; WebRtcAec_Process then takes the
// ProcessExtended path (echo_cancellation.c:377-394).  Like the reference call it belongs right after Init; used
// mid-stream, the streams' states are carried over (re-packed into blocks of the new size) and behave as the
// reference's do, except that the far-spectrum and filter partitions 12..31 are dropped when the filter is
// shortened (the reference leaves them in place, stale, for a later re-enable).
int AspAecBatch_enable_delay_correction(AspAecBatch* b, int enable) {
  AspDeviceScope dev_scope_;
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  const int np = enable ? kNumPartMax : kNumPartNormal;
  if (vmode(b) && np != b->su.num_part)
    return aec_fail(ASP_ERR_STATE, "enable_delay_correction: the streams have their own control planes; Init the batch first");
  if (np != b->su.num_part) {
    if (b->ctl.xf_pos >= np) {
      // the reference keeps running with the large block position (aec_core.c:1876-1881 stores the flag only); the
      // 12-partition state block has no rows 12..31, so the switch is refused until the position is below 12
      // (include/asp_aec.h); the error code tells a caller of the void drop-in wrapper
      b->ctl.lastError = AEC_UNSUPPORTED_FUNCTION_ERROR;
      return aec_fail(ASP_ERR_STATE, "enable_delay_correction(0): xfBufBlockPos is beyond the 12-partition filter; feed frames until it is below 12");
    }
    DeviceIssuer iss(b, DeviceIssuer::kLaunch);
    if (const int rc = flush_pending_farend(b->su, iss)) return rc;
    if (!control_only(b)) {
      AEC_TRY(dev_scope_.select(b->device));
      AEC_TRY(hipStreamSynchronize(b->stream));
      const int od = state_dwords(b), nd = AecRows(np).state_dwords;
      std::vector<float> old_all((size_t)b->S * od), new_all((size_t)b->S * nd);
      AEC_TRY(hipMemcpy(old_all.data(), b->state, old_all.size() * sizeof(float), hipMemcpyDeviceToHost));
      std::vector<AspAecState> canon(1);
      for (int s = 0; s < b->S; ++s) {
        unpack_stream(b->su.num_part, b->ctl, old_all.data() + (size_t)s * od, canon.data());
        pack_stream(np, b->ctl, canon.data(), new_all.data() + (size_t)s * nd);
        keep_rings(new_all.data() + (size_t)s * nd, old_all.data() + (size_t)s * od);
      }
      AEC_TRY(hipFree(b->state));
      b->state = nullptr;
      b->su.num_part = np;
      AEC_TRY(hipMalloc((void**)&b->state, state_bytes(b)));
      AEC_TRY(hipMemcpy(b->state, new_all.data(), new_all.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    b->su.num_part = np;
  }
  b->su.extended = enable;  // the reference stores the argument as given
  if (!control_only(b)) {  // WebRtc_set_allowed_offset(delay_estimator, num_partitions / 2), aec_core.c:1880
    std::vector<int32_t> v((size_t)b->S, b->su.num_part / 2);
    AEC_TRY(dev_scope_.select(b->device));
    AEC_TRY(hipStreamSynchronize(b->stream));
    AEC_TRY(hipMemcpy2D(reinterpret_cast<char*>(b->dblocks) + offsetof(DelayBlock, s.allowed_offset), sizeof(DelayBlock), v.data(),
                        sizeof(int32_t), sizeof(int32_t), (size_t)b->S, hipMemcpyHostToDevice));
  }
  return 0;
}

// WebRtcAec_enable_reported_delay(WebRtcAec_aec_core(inst), enable) for every stream (aec_core.c:1868-1874).
// enable = 0 is the delay-agnostic mode: EstBufDelay is skipped and WebRtcAec_ProcessFrames steers the far-end read
// pointer by the delay estimator (which runs when delay logging is on) instead of the reported delay -- per stream,
// on the device.  Once streams have moved apart, switching the reported delays back on needs a new Init.
int AspAecBatch_enable_reported_delay(AspAecBatch* b, int enable) {
  AspDeviceScope dev_scope_;
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (enable && !b->su.reported_delay_enabled && b->su.agn_synced)
    return aec_fail(ASP_ERR_STATE, "enable_reported_delay: the streams' far buffers have moved apart; Init first");
  // the delay-agnostic mode steers every stream's far buffer on the device: a control-only handle refuses it here,
  // not in the middle of a later Process call with its ring positions already advanced
  if (!enable && control_only(b)) return aec_fail(ASP_ERR_STATE, "enable_reported_delay(0): the delay-agnostic mode needs the device");
  if (!enable && vmode(b))
    return aec_fail(ASP_ERR_STATE, "enable_reported_delay(0): per-stream control covers the reported-delay mode; Init the batch first");
  b->su.reported_delay_enabled = enable ? 1 : 0;
  return 0;
}
int AspAecBatch_reported_delay_enabled(const AspAecBatch* b) { return b ? b->su.reported_delay_enabled : 0; }

// The delay estimator's state of one stream with the stream's far-buffer read side and system delay.
int AspAecBatch_ExportDelayState(AspAecBatch* b, int stream, AspAecDelayState* out) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_ExportDelayState: control-only handle");
  if (!b || !out || stream < 0 || stream >= b->S) return aec_fail(ASP_ERR_PARAM, "ExportDelayState: bad argument");
  AEC_TRY(dev_scope_.select(b->device));
  if (b->su.agn_synced && b->su.nevents > 0) {  // far-end calls the streams' read sides have not seen yet
    DeviceIssuer iss(b, DeviceIssuer::kLaunch);
    if (const int rc = flush_far_events(b->su, iss)) return rc;
  }
  AEC_TRY(hipStreamSynchronize(b->stream));
  AEC_TRY(hipMemcpy(out, &b->dblocks[stream].s, sizeof *out, hipMemcpyDeviceToHost));
  if (!b->su.agn_synced) {  // lock-step: the batch's values
    const AecCtl& c = ctl0(b);
    out->far_read = c.far_pos.read;
    out->far_write = c.far_pos.write;
    out->far_wrap = c.far_pos.wrap;
    out->system_delay = c.system_delay;
  }
  return ASP_OK;
}

// WebRtcAec_GetDelayMetrics for every stream (echo_cancellation.c:550-571, aec_core.c:1780-1836): median and
// spread (L1 norm around the median) of the block-wise delay estimates since the last call, in ms; the
// histograms are cleared.  median / std [num_streams].
int AspAecBatch_GetDelayMetrics(AspAecBatch* b, int* median, int* std) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_GetDelayMetrics: control-only handle");
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (median == nullptr || std == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  if (b->su.delay_logging == 0) return set_error(b, AEC_UNSUPPORTED_FUNCTION_ERROR);  // logging disabled
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  constexpr int H = ASP_AEC_DELAY_HISTORY;
  std::vector<int32_t> hist((size_t)b->S * H), look((size_t)b->S);
  AEC_TRY(hipMemcpy2D(hist.data(), H * sizeof(int32_t), reinterpret_cast<char*>(b->dblocks) + offsetof(DelayBlock, s.delay_histogram),
                      sizeof(DelayBlock), H * sizeof(int32_t), (size_t)b->S, hipMemcpyDeviceToHost));
  AEC_TRY(hipMemcpy2D(look.data(), sizeof(int32_t), reinterpret_cast<char*>(b->dblocks) + offsetof(DelayBlock, s.lookahead),
                      sizeof(DelayBlock), sizeof(int32_t), (size_t)b->S, hipMemcpyDeviceToHost));
  const int kMsPerBlock = kPartLen / (b->su.mult * 8);
  for (int s = 0; s < b->S; ++s) {
    const int32_t* h = hist.data() + (size_t)s * H;
    int num_delay_values = 0, my_median = 0;
    for (int i = 0; i < H; i++) num_delay_values += h[i];
    if (num_delay_values == 0) {
      median[s] = -1;
      std[s] = -1;
      continue;
    }
    int delay_values = num_delay_values >> 1;
    for (int i = 0; i < H; i++) {
      delay_values -= h[i];
      if (delay_values < 0) {
        my_median = i;
        break;
      }
    }
    median[s] = (my_median - look[s]) * kMsPerBlock;
    float l1_norm = 0;
    for (int i = 0; i < H; i++) l1_norm += (float)abs(i - my_median) * h[i];
    std[s] = (int)(l1_norm / (float)num_delay_values + 0.5f) * kMsPerBlock;
  }
  // (a stream without values keeps its -- empty -- histogram; the others are cleared: aec_core.c:1833)
  AEC_TRY(hipMemset2DAsync(reinterpret_cast<char*>(b->dblocks) + offsetof(DelayBlock, s.delay_histogram), sizeof(DelayBlock), 0,
                           H * sizeof(int32_t), (size_t)b->S, b->stream));
  AEC_TRY(hipStreamSynchronize(b->stream));
  return 0;
}

int AspAecBatch_delay_correction_enabled(const AspAecBatch* b) { return b ? b->su.extended : 0; }

int AspAecBatch_GetControl(const AspAecBatch* b, AspAecControl* c) {
  if (!b || !c) return aec_fail(ASP_ERR_PARAM, "GetControl: bad argument");
  fill_control(ctl_of(b, 0), c);
  return ASP_OK;
}

static void fill_control(const AecCtl& k, AspAecControl* c) {
  c->startup_phase = k.startup_phase;
  c->checkBuffSize = k.checkBuffSize;
  c->bufSizeStart = k.bufSizeStart;
  c->knownDelay = k.knownDelay;
  c->filtDelay = k.filtDelay;
  c->timeForDelayChange = k.timeForDelayChange;
  c->lastDelayDiff = k.lastDelayDiff;
  c->counter = k.counter;
  c->sum = k.sum;
  c->firstVal = k.firstVal;
  c->checkBufSizeCtr = k.checkBufSizeCtr;
  c->system_delay = k.system_delay;
  c->core_knownDelay = k.core_knownDelay;
  c->far_read = k.far_pos.read;
  c->far_write = k.far_pos.write;
  c->far_wrap = k.far_pos.wrap;
  c->pre_read = k.pre_pos.read;
  c->pre_write = k.pre_pos.write;
  c->pre_wrap = k.pre_pos.wrap;
  c->near_read = k.near_pos.read;
  c->near_write = k.near_pos.write;
  c->near_wrap = k.near_pos.wrap;
  c->out_read = k.out_pos.read;
  c->out_write = k.out_pos.write;
  c->out_wrap = k.out_pos.wrap;
  c->blocks_processed = k.blocks_processed;
}

int AspAecBatch_get_echo_status(AspAecBatch* b, int* status) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_get_echo_status: control-only handle");
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (status == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  for (int s = 0; s < b->S; ++s) {
    int32_t v = 0;
    AEC_TRY(hipMemcpy(&v, b->state + (size_t)s * state_dwords(b) + kOffScalars + S_ECHOSTATE, sizeof v, hipMemcpyDeviceToHost));
    status[s] = v;
  }
  return 0;
}

namespace {
void level_of(const AspAecStats& s, AecLevel* out) {  // echo_cancellation.c:484-499 (and the erle / aNlp copies)
  const float kUpWeight = 0.7f;
  out->instant = (int)s.instant;
  if ((s.himean > -100) && (s.average > -100)) {
    const float dtmp = kUpWeight * s.himean + (1 - kUpWeight) * s.average;
    out->average = (int)dtmp;
  } else {
    out->average = -100;
  }
  out->max = (int)s.max;
  out->min = s.min < 100 ? (int)s.min : -100;
}
}  // namespace

int AspAecBatch_GetMetrics(AspAecBatch* b, AecMetrics* out) {  // WebRtcAec_GetMetrics, echo_cancellation.c:456-548
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_GetMetrics: control-only handle");
  if (!b) return aec_fail(ASP_ERR_PARAM, "null batch handle");
  if (out == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  std::vector<float> all((size_t)b->S * kMetDwords);
  AEC_TRY(hipMemcpy(all.data(), b->metrics, all.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int s = 0; s < b->S; ++s) {
    AspAecMetricsState m;
    memcpy(&m, all.data() + (size_t)s * kMetDwords, sizeof m);
    AecMetrics* o = out + s;
    level_of(m.erl, &o->erl);
    level_of(m.erle, &o->erle);
    const int stmp = (o->erl.average > -100 && o->erle.average > -100) ? o->erl.average + o->erle.average : -100;
    o->rerl.average = stmp;
    o->rerl.instant = stmp;
    o->rerl.max = stmp;
    o->rerl.min = stmp;
    level_of(m.aNlp, &o->aNlp);
  }
  return 0;
}

int AspAecBatch_ExportMetricsState(AspAecBatch* b, int stream, AspAecMetricsState* out) {
  AspDeviceScope dev_scope_;
  if (b && control_only(b)) return aec_fail(ASP_ERR_STATE, "AspAecBatch_ExportMetricsState: control-only handle");
  if (!b || !out || stream < 0 || stream >= b->S) return aec_fail(ASP_ERR_PARAM, "ExportMetricsState: bad argument");
  AEC_TRY(dev_scope_.select(b->device));
  AEC_TRY(hipStreamSynchronize(b->stream));
  AEC_TRY(hipMemcpy(out, b->metrics + (size_t)stream * kMetDwords, sizeof *out, hipMemcpyDeviceToHost));
  return 0;
}

// Diagnostic: one BufferFarend + Process on device frames with phase time stamps (s_memtime
// ticks) of stream 0's first block.
int AspAecBatch_DebugStamps(AspAecBatch* b, const float* far_dev, const float* near_dev, float* out_dev,
                            unsigned long long* stamps16) {
  AspDeviceScope dev_scope_;
  if (!b || !far_dev || !near_dev || !out_dev || !stamps16) return aec_fail(ASP_ERR_PARAM, "DebugStamps: bad argument");
  AEC_TRY(dev_scope_.select(b->device));
  unsigned long long* d = nullptr;
  AEC_TRY(hipMalloc((void**)&d, 16 * sizeof(unsigned long long)));
  hipError_t e = hipMemset(d, 0, 16 * sizeof(unsigned long long));
  int err = 0, rc = 0;
  if (e == hipSuccess) {
    DeviceIssuer iss(b, DeviceIssuer::kLaunch, 0, d);
    iss.near = near_dev;
    iss.out = out_dev;
    err = buffer_farend_device(b->su, b->ctl, iss, far_dev, 160);
    if (err == 0) err = process_device(b->su, b->ctl, iss, 160, 0, &rc);
    e = hipStreamSynchronize(b->stream);
  }
  if (e == hipSuccess) e = hipMemcpy(stamps16, d, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return aec_fail(ASP_ERR_HIP, "DebugStamps", e);
  return err;
}

int AspAec_rdft128_batch(const float* src, float* dst, int isgn, int count, int device) {
  AspDeviceScope dev_scope_;
  if (!src || !dst || count <= 0) return aec_fail(ASP_ERR_PARAM, "rdft128_batch: bad argument");
  // an ordinal out of range is reported as the HIP failure it has always been
  if (int rc = dev_scope_.select("asp_aec", device, ASP_ERR_HIP, "no HIP device: the echo canceller has no CPU fallback")) return rc;
  float *d_in = nullptr, *d_out = nullptr;
  AecTables* d_t = nullptr;
  const size_t bytes = (size_t)count * 128 * sizeof(float);
  AecTables T;
  build_tables(&T);
  hipError_t e = hipMalloc((void**)&d_in, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&d_t, sizeof T);
  if (e == hipSuccess) e = hipMemcpy(d_t, &T, sizeof T, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_in, src, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_aec_rdft128(d_in, d_out, isgn, count, d_t, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(dst, d_out, bytes, hipMemcpyDeviceToHost);
  if (d_in) (void)hipFree(d_in);
  if (d_out) (void)hipFree(d_out);
  if (d_t) (void)hipFree(d_t);
  if (e != hipSuccess) return aec_fail(ASP_ERR_HIP, "rdft128_batch", e);
  return ASP_OK;
}

int AspAec_delay_estimator_batch(AspAecDelayState* states, int count, const uint32_t* binary_far, const uint32_t* binary_near,
                                 int nblocks, int device) {
  AspDeviceScope dev_scope_;
  if (!states || !binary_far || !binary_near || count <= 0 || nblocks < 0)
    return aec_fail(ASP_ERR_PARAM, "delay_estimator_batch: bad argument");
  // an ordinal out of range is reported as the HIP failure it has always been
  if (int rc = dev_scope_.select("asp_aec", device, ASP_ERR_HIP, "no HIP device: the echo canceller has no CPU fallback")) return rc;
  std::vector<DelayBlock> blocks((size_t)count);
  for (int i = 0; i < count; ++i) {
    memset(&blocks[i], 0, sizeof(DelayBlock));
    blocks[i].s = states[i];
  }
  std::vector<unsigned> words((size_t)count * kFlowBitsBlocks * 2);
  DelayBlock* d_blocks = nullptr;
  unsigned* d_bits = nullptr;
  hipError_t e = hipMalloc((void**)&d_blocks, blocks.size() * sizeof(DelayBlock));
  if (e == hipSuccess) e = hipMalloc((void**)&d_bits, words.size() * sizeof(unsigned));
  if (e == hipSuccess) e = hipMemcpy(d_blocks, blocks.data(), blocks.size() * sizeof(DelayBlock), hipMemcpyHostToDevice);
  for (int k0 = 0; k0 < nblocks && e == hipSuccess; k0 += kFlowBitsBlocks) {  // as many launches as hand-off launches would carry
    const int nb = nblocks - k0 < kFlowBitsBlocks ? nblocks - k0 : kFlowBitsBlocks;
    for (int i = 0; i < count; ++i)
      for (int k = 0; k < nb; ++k) {
        words[((size_t)i * kFlowBitsBlocks + k) * 2] = binary_far[(size_t)i * nblocks + k0 + k];
        words[((size_t)i * kFlowBitsBlocks + k) * 2 + 1] = binary_near[(size_t)i * nblocks + k0 + k];
      }
    e = hipMemcpy(d_bits, words.data(), words.size() * sizeof(unsigned), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_aec_delay_bits(d_blocks, d_bits, count, nb, 1, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e == hipSuccess) e = hipMemcpy(blocks.data(), d_blocks, blocks.size() * sizeof(DelayBlock), hipMemcpyDeviceToHost);
  if (d_blocks) (void)hipFree(d_blocks);
  if (d_bits) (void)hipFree(d_bits);
  if (e != hipSuccess) return aec_fail(ASP_ERR_HIP, "delay_estimator_batch", e);
  for (int i = 0; i < count; ++i) states[i] = blocks[i].s;
  return ASP_OK;
}

int AspAec_host_table(int which, float* out, int capacity) {
  AspDeviceScope dev_scope_;
  AecTables T;
  build_tables(&T);
  const float* src = nullptr;
  int n = 0;
  switch (which) {
    case 0: src = T.w; n = 64; break;
    case 1: src = T.wk3a; n = 16; break;
    case 2: src = T.wk3b; n = 16; break;
    case 3: src = T.hann; n = 65; break;
    case 4: src = T.weight; n = 65; break;
    case 5: src = T.odrive; n = 65; break;
    default: return aec_fail(ASP_ERR_PARAM, "host_table: unknown table");
  }
  if (!out || capacity < n) return aec_fail(ASP_ERR_PARAM, "host_table: buffer too small");
  memcpy(out, src, n * sizeof(float));
  return n;
}

// ------------------------------------------------------------------ layer 1
// The reference's per-stream API: a handle is a batch of one stream, host buffers.
int32_t WebRtcAec_Create(void** aecInst) {  // echo_cancellation.c:121-168
  if (aecInst == nullptr) return -1;
  AspAecBatch* b = nullptr;
  if (AspAecBatch_Create(&b, 1, 0) != ASP_OK) {
    *aecInst = nullptr;
    return -1;
  }
  *aecInst = b;
  return 0;
}

int32_t WebRtcAec_Free(void* aecInst) {
  AspDeviceScope dev_scope_;
  if (aecInst == nullptr) return -1;
  return AspAecBatch_Free((AspAecBatch*)aecInst);
}

int32_t WebRtcAec_Init(void* aecInst, int32_t sampFreq, int32_t scSampFreq) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_Init((AspAecBatch*)aecInst, sampFreq, scSampFreq) == 0 ? 0 : -1;
}

int32_t WebRtcAec_BufferFarend(void* aecInst, const float* farend, int16_t nrOfSamples) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_BufferFarend((AspAecBatch*)aecInst, farend, nrOfSamples, ASP_MEM_HOST) == 0 ? 0 : -1;
}

int32_t WebRtcAec_Process(void* aecInst, const float* const* nearend, int num_bands,
                          float* const* out, int16_t nrOfSamples, int16_t msInSndCardBuf,
                          int32_t skew) {
  AspDeviceScope dev_scope_;
  AspAecBatch* b = (AspAecBatch*)aecInst;
  if (b == nullptr) return -1;
  if (out == nullptr || nearend == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  // the reference asserts aec->num_bands == num_bands (aec_core.c:1683)
  if (num_bands != 1 + b->su.num_high) return set_error(b, AEC_BAD_PARAMETER_ERROR);
  if (num_bands == 2)
    return AspAecBatch_ProcessBands(b, nearend[0], nearend[1], out[0], out[1], nrOfSamples, msInSndCardBuf,
                                    skew, ASP_MEM_HOST) == 0 ? 0 : -1;
  return AspAecBatch_Process(b, nearend[0], out[0], nrOfSamples, msInSndCardBuf, skew, ASP_MEM_HOST) == 0 ? 0 : -1;
}

int WebRtcAec_set_config(void* handle, AecConfig config) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_set_config((AspAecBatch*)handle, config) == 0 ? 0 : -1;
}

int WebRtcAec_get_echo_status(void* handle, int* status) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_get_echo_status((AspAecBatch*)handle, status) == 0 ? 0 : -1;
}

int WebRtcAec_GetMetrics(void* handle, AecMetrics* metrics) {  // echo_cancellation.c:456-548
  AspAecBatch* b = (AspAecBatch*)handle;
  if (b == nullptr) return -1;
  if (metrics == nullptr) return set_error(b, AEC_NULL_POINTER_ERROR);
  if (b->su.initFlag != kInitCheck) return set_error(b, AEC_UNINITIALIZED_ERROR);
  return AspAecBatch_GetMetrics(b, metrics) == 0 ? 0 : -1;
}

int WebRtcAec_GetDelayMetrics(void* handle, int* median, int* std) {  // echo_cancellation.c:550-571
  AspAecBatch* b = (AspAecBatch*)handle;
  if (b == nullptr) return -1;
  return AspAecBatch_GetDelayMetrics(b, median, std) == 0 ? 0 : -1;
}

int32_t WebRtcAec_get_error_code(void* aecInst) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_get_error_code((AspAecBatch*)aecInst);
}

struct AecCore* WebRtcAec_aec_core(void* handle) {
  AspDeviceScope dev_scope_;
  return reinterpret_cast<struct AecCore*>(handle);
}

// aec_core.h:129-133 / aec_core.c:1876-1885: `self` is the token WebRtcAec_aec_core returned
void WebRtcAec_enable_delay_correction(struct AecCore* self, int enable) {
  AspDeviceScope dev_scope_;
  (void)AspAecBatch_enable_delay_correction(reinterpret_cast<AspAecBatch*>(self), enable);
}

int WebRtcAec_delay_correction_enabled(struct AecCore* self) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_delay_correction_enabled(reinterpret_cast<AspAecBatch*>(self));
}

// aec_core.h:110-114 / aec_core.c:1886-1894 (what echo_cancellation_unittest.cc:34-48 and the APM use): the buffered
// far-end delay in samples.  In the delay-agnostic mode it is the stream's own (a handle is a batch of one stream).
int WebRtcAec_system_delay(struct AecCore* self) {
  AspDeviceScope dev_scope_;
  AspAecBatch* b = reinterpret_cast<AspAecBatch*>(self);
  if (!b) return 0;
  if (b->su.agn_synced && !control_only(b)) {
    AspAecDelayState d;
    if (AspAecBatch_ExportDelayState(b, 0, &d) == ASP_OK) return d.system_delay;
  }
  return ctl0(b).system_delay;
}
void WebRtcAec_SetSystemDelay(struct AecCore* self, int delay) {
  AspDeviceScope dev_scope_;
  AspAecBatch* b = reinterpret_cast<AspAecBatch*>(self);
  if (!b || delay < 0) return;  // the reference asserts delay >= 0
  ctl0(b).system_delay = delay;
  if (b->su.agn_synced && !control_only(b)) {
    std::vector<int32_t> v((size_t)b->S, delay);
    if (dev_scope_.select(b->device) != hipSuccess || hipStreamSynchronize(b->stream) != hipSuccess) return;
    (void)hipMemcpy2D(reinterpret_cast<char*>(b->dblocks) + offsetof(DelayBlock, s.system_delay), sizeof(DelayBlock), v.data(),
                      sizeof(int32_t), sizeof(int32_t), (size_t)b->S, hipMemcpyHostToDevice);
  }
}

// aec_core.h:121-126 / aec_core.c:1868-1874
void WebRtcAec_enable_reported_delay(struct AecCore* self, int enable) {
  AspDeviceScope dev_scope_;
  (void)AspAecBatch_enable_reported_delay(reinterpret_cast<AspAecBatch*>(self), enable);
}

int WebRtcAec_reported_delay_enabled(struct AecCore* self) {
  AspDeviceScope dev_scope_;
  return AspAecBatch_reported_delay_enabled(reinterpret_cast<AspAecBatch*>(self));
}

}  // extern "C"
