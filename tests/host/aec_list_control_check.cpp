// aec_list_control_check.cpp -- the planning step of the AEC list calls (csrc/aec_control.h, plan_list) without the
// HIP library: a stand-alone program for a sanitizer build (tests/test_aec_list_control_host.py builds it with ASan +
// UBSan and runs it).  argv[1] names the schedule of tests/aec_list_cases.py as text: the stream count, the per-stream
// delays, then per tick the entry count and the entries' (stream, count) pairs.  Every tick is planned the way
// AspAecBatch_RunList plans it -- on copies of the listed streams' control planes, one launch's frames at a time, the
// copies committed after each launch -- with a sink that checks every descriptor against the bounds aec_list_kernel
// relies on, and into a [entry][frame] array of exactly the size the library stages.  Three configurations: 16 kHz /
// 160 samples, 8 kHz / 80 samples, the extended filter.  Prints one line of totals; exit status 0 = every bound held.
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

struct CheckSink final : AecListSink {
  const AecSetup& su;
  int n = 0, nr = 0, stride = 0;
  const int32_t* left = nullptr;         // [n]: the entries' frames in this launch
  std::vector<AecListStep> descs;        // [n][stride], as staged
  std::vector<int> next;                 // [n]: the frame each entry must hand over next
  long steps = 0, passes = 0, blocks = 0, parts = 0, appends_only = 0;
  explicit CheckSink(const AecSetup& su_) : su(su_) {}

  void begin(int n_, int nr_, int stride_, const int32_t* left_) {
    n = n_;
    nr = nr_;
    stride = stride_;
    left = left_;
    CHECK(in(stride, 1, kAecListMaxFrames + 1));
    descs.assign((size_t)n * stride, AecListStep{});
    next.assign((size_t)n, 0);
  }
  int step(int entry, int frame, const AecListStep& d) override {
    CHECK(in(entry, 0, n) && in(frame, 0, left[entry]) && frame == next[(size_t)entry]);  // in order, none twice
    ++next[(size_t)entry];
    descs[(size_t)entry * stride + frame] = d;
    // far end: the ring indices farend_work forms, the slots it writes
    const FarOps& fo = d.far;
    CHECK((fo.n == nr || fo.n == 0) && in(fo.wpos, 0, kPreLen + 1) && in(fo.nparts, 0, 4));
    for (int i = 0; i < fo.nparts; ++i) CHECK(in(fo.rpos[i], 0, kPreLen + 1) && in(fo.slot[i], 0, kFarSlots));
    parts += fo.nparts;
    appends_only += fo.nparts == 0;
    CHECK(d.mode == 0 || d.mode == 1);
    ++steps;
    if (d.mode == 0) {
      ++passes;
      return 0;
    }
    const ProcOps& ops = d.ops;
    CHECK(in(ops.nsub, 1, 3) && ops.nsub == nr / kFrameLen);
    CHECK(ops.mult == su.mult && ops.num_high == 0 && ops.nlp_mode == su.nlp_mode && !ops.spectra && !ops.agnostic);
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
    return 0;
  }
  void end() {
    for (int i = 0; i < n; ++i) CHECK(next[(size_t)i] == left[i]);  // every frame of the launch has its descriptor
  }
};

void check_ring(const RingPos& r, int count) {
  CHECK(r.count == count && in(r.read, 0, count + 1) && in(r.write, 0, count + 1) && in(r.wrap, 0, 2));
  CHECK(in(rp_avail_read(&r), 0, count + 1));
}

struct Tick {
  std::vector<int32_t> streams, counts;
};

}  // namespace

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp != nullptr);
  int S = 0;
  CHECK(fscanf(fp, "%d", &S) == 1 && in(S, 1, 4097));
  std::vector<int> delays((size_t)S);
  for (int& d : delays) CHECK(fscanf(fp, "%d", &d) == 1);
  std::vector<Tick> ticks;
  for (int n; fscanf(fp, "%d", &n) == 1;) {
    CHECK(in(n, 0, S + 1));
    Tick t;
    for (int i = 0; i < n; ++i) {
      int s, c;
      CHECK(fscanf(fp, "%d %d", &s, &c) == 2 && in(s, 0, S) && c >= 0);
      t.streams.push_back(s);
      t.counts.push_back(c);
    }
    ticks.push_back(t);
  }
  fclose(fp);
  CHECK(!ticks.empty());

  long frames = 0, steps = 0, passes = 0, blocks = 0, parts = 0, appends_only = 0, launches = 0, cut_calls = 0;
  const int rows[3][3] = {{16000, 160, 0}, {8000, 80, 0}, {16000, 160, 1}};
  for (const auto& row : rows) {
    AecSetup su;
    AecCtl c0;
    init_control(su, c0, row[0], 48000);
    if (row[2]) {  // AspAecBatch_enable_delay_correction(1)
      su.extended = 1;
      su.num_part = kNumPartMax;
    }
    const int nr = row[1];
    std::vector<AecCtl> per((size_t)S, c0);
    CheckSink sink(su);
    // the schedule as it stands, then once more with every count times five: calls that are cut into launches
    for (int pass = 0; pass < 2; ++pass) {
      for (const Tick& t : ticks) {
        const int n = (int)t.streams.size();
        std::vector<int32_t> counts(t.counts);
        for (int32_t& c : counts) c *= pass ? 5 : 1;
        int maxc = 0;
        for (int32_t c : counts) maxc = c > maxc ? c : maxc;
        std::vector<AecCtl> work((size_t)n);
        std::vector<int16_t> ms((size_t)n);
        std::vector<int32_t> status((size_t)n, 0), left((size_t)n);
        for (int i = 0; i < n; ++i) {
          work[(size_t)i] = per[(size_t)t.streams[(size_t)i]];
          ms[(size_t)i] = (int16_t)delays[(size_t)t.streams[(size_t)i]];
        }
        cut_calls += maxc > kAecListMaxFrames;
        for (int f0 = 0; f0 < maxc; f0 += kAecListMaxFrames, ++launches) {
          const int nf = maxc - f0 < kAecListMaxFrames ? maxc - f0 : kAecListMaxFrames;
          for (int i = 0; i < n; ++i) {
            const int l = counts[(size_t)i] - f0;
            left[(size_t)i] = l < 0 ? 0 : l < nf ? l : nf;
            frames += left[(size_t)i];
          }
          sink.begin(n, nr, nf, left.data());
          CHECK(plan_list(su, work.data(), counts.data(), n, f0, nf, nr, ms.data(), status.data(), sink) == 0);
          sink.end();
          for (int i = 0; i < n; ++i) per[(size_t)t.streams[(size_t)i]] = work[(size_t)i];
        }
        for (int i = 0; i < n; ++i) CHECK(status[(size_t)i] == 0);
        for (const AecCtl& c : per) {
          check_ring(c.pre_pos, kPreLen);
          check_ring(c.far_pos, kFarSlots);
          check_ring(c.near_pos, kFrBufLen);
          check_ring(c.out_pos, kFrBufLen);
          CHECK(in(c.xf_pos, 0, su.num_part) && in(c.xfw_head, 0, kNumPartMax));
        }
      }
    }
    // start-up and the running phase were both there (ProcessExtended leaves start-up in its first call: no pass-through)
    CHECK((sink.passes > 0 || row[2]) && sink.blocks > 0);
    steps += sink.steps;
    passes += sink.passes;
    blocks += sink.blocks;
    parts += sink.parts;
    appends_only += sink.appends_only;
  }
  CHECK(steps == frames && cut_calls > 0);
  printf("aec_list_control_check: %ld frames in %ld launches (%ld calls cut), %ld pass-throughs, %ld blocks, %ld far "
         "partitions, %ld frames that only append: all bounds held\n",
         frames, launches, cut_calls, passes, blocks, parts, appends_only);
  return 0;
}
