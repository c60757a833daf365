// aec_control_check.cpp -- the AEC host control plane (csrc/aec_control.h) without the HIP library: a stand-alone
// program for a sanitizer build (tests/test_aec_control_host.py builds it with ASan + UBSan and runs it).  Its issuer
// launches nothing; it checks every descriptor the control plane hands over against the bounds the kernels rely on.
// Driven with the call sequences of tests/test_aec_oracle.py: the seven lock-step rows of
// test_host_control_plane_matches_oracle and the twelve-stream schedule of
// test_per_stream_control_plane_matches_oracle.  Prints one line of totals; exit status 0 = every bound held.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "aec_control.h"
#include "asp_ns.h"  // ASP_ERR_STATE

using namespace aspaec;

int aspaec::aec_refuse(const char* what) {
  fprintf(stderr, "refused: %s\n", what);
  return ASP_ERR_STATE;
}

namespace {

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: bound broken: %s\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

bool in(int v, int lo, int hi) { return v >= lo && v < hi; }

struct CheckIssuer final : AecIssuer {
  const AecSetup& su;
  long farends = 0, processes = 0, blocks = 0, passes = 0, delays = 0, resamples = 0;
  std::vector<float> resampled = std::vector<float>(kResamplerBufferSize);
  explicit CheckIssuer(const AecSetup& su_) : su(su_) {}

  void check_far(const FarOps& ops) {
    CHECK(in(ops.n, 0, kPreLen + 1) && in(ops.wpos, 0, kPreLen + 1) && in(ops.nparts, 0, 4));
    for (int i = 0; i < ops.nparts; ++i) CHECK(in(ops.rpos[i], 0, kPreLen + 1) && in(ops.slot[i], 0, kFarSlots));
  }
  int farend(const float* far, const FarOps& ops) override {
    CHECK(far != nullptr);
    check_far(ops);
    ++farends;
    return 0;
  }
  int process(int n, const ProcOps& ops, const float* far_src, const FarOps& fops, const AgnOps* agn, int sub) override {
    CHECK((n == 80 || n == 160) && in(ops.nsub, 1, 3) && ops.nsub <= n / kFrameLen && in(sub, -1, 2));
    CHECK(ops.mult == su.mult && ops.num_high == su.num_high && ops.nlp_mode == su.nlp_mode);
    for (int j = 0; j < ops.nsub; ++j) {
      const SubFrame& sf = ops.sub[j];
      CHECK(in(sf.nblocks, 0, 3) && in(sf.near_wpos, 0, kFrBufLen + 1) && in(sf.out_rpos, 0, kFrBufLen + 1));
      for (int k = 0; k < sf.nblocks; ++k) {
        const BlockOp& op = sf.blk[k];
        CHECK(in(op.near_rpos, 0, kFrBufLen + 1) && in(op.out_wpos, 0, kFrBufLen + 1) && in(op.far_slot, 0, kFarSlots));
        CHECK(in(op.xf_pos, 0, su.num_part) && in(op.xfw_head, 0, kNumPartMax));
        ++blocks;
      }
    }
    if (far_src) check_far(fops);
    if (agn)
      for (int j = 0; j < ops.nsub; ++j) CHECK(delay(agn->sub[j]) == 0);
    ++processes;
    return 0;
  }
  int pass_through(int n) override {
    CHECK(n == 80 || n == 160);
    ++passes;
    return 0;
  }
  int delay(const DelayOps& d) override {
    CHECK(in(d.nevents, 0, kMaxFarEvents + 1) && in(d.nblocks, 0, 3) && in(d.npending, 0, kSpecBlocks + 1));
    ++delays;
    return 0;
  }
  int resample(const float** far, int n, int n_out, float be, float position) override {
    CHECK((n == 80 || n == 160) && in(n_out, 0, kResamplerBufferSize + 1) && be > 0.f && position >= 0.f);
    *far = resampled.data();
    ++resamples;
    return 0;
  }
};

void check_ring(const RingPos& r, int count) {
  CHECK(r.count == count && in(r.read, 0, count + 1) && in(r.write, 0, count + 1) && in(r.wrap, 0, 2));
  CHECK(in(rp_avail_read(&r), 0, count + 1));
}
void check_ctl(const AecSetup& su, const AecCtl& c) {
  check_ring(c.pre_pos, kPreLen);
  check_ring(c.far_pos, kFarSlots);
  check_ring(c.near_pos, kFrBufLen);
  check_ring(c.out_pos, kFrBufLen);
  CHECK(in(c.xf_pos, 0, su.num_part) && in(c.xfw_head, 0, kNumPartMax));
  CHECK(in(su.nevents, 0, kMaxFarEvents + 1) && in(su.rs_skewDataIndex, 0, kSkewEstimateFrames + 2));
}

void use_extended_filter(AecSetup& su) {  // AspAecBatch_enable_delay_correction(1)
  su.extended = 1;
  su.num_part = kNumPartMax;
}

int frame(AecSetup& su, AecCtl& c, CheckIssuer& iss, const float* far, int n, int delay_ms, int skew) {
  int rc = 0;
  CHECK(buffer_farend_device(su, c, iss, far, n) == 0);
  CHECK(process_device(su, c, iss, n, delay_ms, &rc, skew) == 0);
  check_ctl(su, c);
  return rc;
}

}  // namespace

int main() {
  std::vector<float> far(160, 0.f);
  long frames = 0, warnings = 0, farends = 0, processes = 0, blocks = 0, passes = 0, resamples = 0;
  auto add = [&](const CheckIssuer& i) {
    farends += i.farends;
    processes += i.processes;
    blocks += i.blocks;
    passes += i.passes;
    resamples += i.resamples;
  };
  // the lock-step rows: delay jumps, both call sizes, both rates, the extended filter, skew compensation
  const int rows[7][4] = {{16000, 160, 0, 0}, {16000, 80, 0, 0}, {8000, 80, 0, 0}, {16000, 160, 1, 0},
                          {8000, 80, 1, 0},   {16000, 160, 0, 17}, {8000, 80, 0, -11}};
  for (const auto& row : rows) {
    const int fs = row[0], n = row[1], ext = row[2], skw = row[3];
    AecSetup su;
    AecCtl c;
    init_control(su, c, fs, 48000);
    if (skw) su.skewMode = kAecTrue;
    if (ext) use_extended_filter(su);
    CheckIssuer iss(su);
    for (int f = 0; f < 900; ++f, ++frames) {
      int d = 0;
      if (f == 120 || f == 121) d = 700;
      if (f == 300) d = -3;
      if (400 <= f && f < 520) d = 90;
      if (600 <= f && f < 640) d = 20;
      const int sk = f % 89 ? skw + (f * 7) % 5 - 2 : 4000;
      warnings += frame(su, c, iss, far.data(), n, d, sk) != 0;
    }
    // (a row need not leave the start-up phase: 80-sample calls at 16 kHz never do, as in the reference)
    CHECK(iss.processes + iss.passes == 900 && (skw == 0 || iss.resamples > 0));
    add(iss);
  }
  // per-stream control: twelve streams with their own reported delays, one re-initialised, uniform calls on top
  for (int ext = 0; ext < 2; ++ext) {
    const int S = 12, base[S] = {0, 0, 20, 40, 60, 100, 5, 0, 250, 30, 80, 10};
    AecSetup su;
    AecCtl c0;
    init_control(su, c0, 16000, 48000);
    if (ext) use_extended_filter(su);
    std::vector<AecCtl> per(S, c0);
    CheckIssuer iss(su);
    for (int f = 0; f < 460; ++f) {
      if (f == 170) init_stream_control(per[5]);
      for (int s = 0; s < S; ++s, ++frames) {
        int d = base[s];
        if (s == 1 && f >= 130) d = 90;
        if (s == 4 && 200 <= f && f < 210) d = 700;
        if (s == 7 && f == 250) d = -5;
        if (300 <= f && f < 320) d = 35;
        warnings += frame(su, per[s], iss, far.data(), 160, d, 0) != 0;
      }
    }
    int distinct = 0;
    for (int s = 0; s < S; ++s) {
      bool seen = false;
      for (int t = 0; t < s; ++t) seen |= per[t].far_pos.read == per[s].far_pos.read;
      distinct += !seen;
    }
    CHECK(distinct > 3);  // the streams did move apart
    add(iss);
  }
  printf("aec_control_check: %ld frames, %ld far-end and %ld process descriptors (%ld blocks), %ld pass-throughs, "
         "%ld resamples, %ld delay warnings: all bounds held\n",
         frames, farends, processes, blocks, passes, resamples, warnings);
  return 0;
}
