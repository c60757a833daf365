// ns_kernels1.hip -- the fused Analyze+Process frame step with ONE stream per wave64 and two
// bins per lane: the low-latency build of the frame step.
//
// Same arithmetic as ns_frame_kernel<true,true> (ns_kernels.hip) -- every per-bin float operation of
// ns_core.c:1043-1359 in the reference's order, Ooura-order FFT (fft4g.c), exact libm forms
// (ns_device.h), the wave-uniform scalar sections of ns_step.h -- mapped so that a frame step of 4096 streams is 4096 short waves, all resident at
// once (four per SIMD at <= 128 VGPRs): a step is bound by the time a wave needs from its first load
// to its last store plus the launch boundary (profiles/README.md, rounds 2 and 3).
//
//   * lane L = 2 lam + h (lam = q + 16 g: the "dual lane" of ns_layout.h's row order) owns the
//     FFT elements / bins E = q + 64 g + 16 t for t = h and t = h + 2: exactly the two outputs
//     of its half of a radix-4 butterfly (outputs 0, 2 on even lanes, 1, 3 on odd lanes), and,
//     with ns_layout.h's row order (t = 0, 2, 1, 3 inside a dual lane), one 8-byte access per
//     state row; bin 128 is computed on every lane (wave-uniform) and committed with the scalars;
//   * per-stream scalars are wave-uniform: read from the scalar row with v_readlane, every
//     data-independent branch of the reference is a scalar branch, written back with v_writelane;
//     the hand-off build's product kernels keep the float scalars and most row tails in the wave's LDS image (ScalarRow);
//   * independent wave-uniform chains with one formula are evaluated ONCE, each on its own lane: bin 128 of the three
//     quantile trackers on lanes 48..50 of the scalar row, the flatness feature's exp beside bin 128's exp(-logLrt) --
//     each value through the operations of its wave-uniform pass (bit-identical), no LDS, no barrier;
//   * the three radix-4 passes go through a 1 KB LDS tile per wave (each lane computes half a
//     butterfly, no duplicated arithmetic), the radix-2 tail through v_permlane32_swap (element p
//     on lane L, p + 64 on lane L ^ 32), the real split through one LDS gather;
//   * cross-bin sums: lane-local (slot A + slot B, + bin 128 on lane 0), then the wave64 xor
//     butterfly of ns_device.h's wave_sum; oracle/ns_oracle.c reproduces this association as
//     ASP_NS_REDUCE_TREE64P and the tests compare bit for bit (outputs and every state array).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "handoff.h"
#include "ns_device.h"
#include "ns_layout.h"
#include "ns_pair_fft.h"
#include "ns_step.h"

namespace {
using namespace asphandoff;
using namespace aspns_dev;
using namespace aspns_pair;

// which CU a wave runs on, for the timeline diagnostic: HW_ID[15:8] (cu_id, sh_id, se_id) and XCC_ID[3:0]
__device__ __forceinline__ unsigned long long ns_cu_tag() {
  const unsigned hw = __builtin_amdgcn_s_getreg((7 << 11) | (8 << 6) | 4);    // HW_REG_HW_ID, bits 8..15
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);  // HW_REG_XCC_ID, bits 0..3
  return (unsigned long long)((xcc << 8) | hw);
}

constexpr int NS3 = 3;  // 2 owned bins + the tail bin 128

// A wave-uniform value parked in a vector register: the diagnostic kernels keep their few extra words there, because
// the step loop of the hand-off build has no scalar register to spare (SGPR spills) and a few vector ones.
template <typename V>
__device__ __forceinline__ V ns_in_vgpr(V x) {
  asm volatile("" : "+v"(x));
  return x;
}

// A copy of a lane constant that the compiler cannot see through.  The rarely taken paths of the frame step (start-up,
// histogram window) derive addresses, masks and fp64 values from the lane index; in the step loop of the hand-off build
// those are loop invariants, hoisted in front of the loop and carried in registers the hot path needs (spills).  Derived
// from ns_cold(x) they are computed where they are used, as in a kernel without the loop.
__device__ __forceinline__ int ns_cold(int x) {
  asm volatile("" : "+v"(x));
  return x;
}
template <typename P>
__device__ __forceinline__ const P* ns_cold(const P* p) {  // (a wave-uniform pointer: its field addresses)
  asm volatile("" : "+s"(p));
  return p;
}

// ---- the hand-off build (FLOW): consecutive frame steps overlap on the chip (the protocol: handoff.h).
// What a stream's walks hand each other is its state block: every state access of this build that reaches memory is
// sc1; `in` / `out` frames and the constant tables stay plain (non-temporal frame accesses were measured and dropped: level with a
// ring of 100 frames, 0.9 us slower per step with a ring of 20, which they keep out of the Infinity Cache:
// profiles/r05_ns_walk_ab.txt).  Step j of a launch reads / writes ring slot (slot0 + j) % ring.
//
// The launch is cut into chunks of `walk` consecutive steps: workgroup (x, c) WALKS steps c walk .. min(steps, (c + 1)
// walk) - 1 of its four streams, one after the other.  What does not change from step to step -- the tables in LDS and
// the one barrier behind them, the lane constants, the stream's buffer descriptor -- is set up once per chunk, and only
// the chunk's first step waits for a counter.  walk == 1 is one step per workgroup; walk == steps leaves no dependency
// between workgroups at all -- and every wave of the chip in the same phase again.  The host sizes the walk to the
// launch (ns_api.hip, flow_walk_auto): 8 steps for a batch with at least one workgroup per compute unit, 4 for a smaller
// one -- every chunk boundary costs the image's write-back, the drain, the publish, the exit skew of the workgroup's
// four waves and the successor's set-up and copy-in, which the resident state block below made the larger part of what
// a walk saves; 16 steps and more lose again where the last round of workgroups is ragged (profiles/README.md).
//
// The resident state block: nobody else may touch a stream's state before its walk ends, so the hot part of the block
// -- its first kImgDwords dwords in ns_layout.h order: scalars and row tails, both sliding-buffer carries, rows V_LQ0 ..
// V_AVGPAUSE -- lives in an LDS image of the wave for the length of the walk.  The wave copies it in once behind the
// chunk's wait, every step goes through the image (StateAcc), and after the walk's last step the wave writes the image
// back (sc1), drains and publishes seq[stream] = want + (the walk's end): once per walk.  Between two of its own steps
// a wave neither drains nor publishes; the scalar row's integer slots stay in its register, the float ones in the image
// (ScalarRow).  What stays in memory inside a walk -- the
// start-up rows V_INITMAGN / V_PARAMNOISE and the histograms -- is read back only in rare paths, which wait for the
// wave's outstanding stores themselves.  Each wave touches only its own image: no barrier is added.
struct NsFlowArgs {
  HandoffArgs hand;
  unsigned want;      // step 0 of the launch is step `want` of every stream (seq[s] == want on entry; a walk over
                      // steps j .. e - 1 of the launch leaves seq[s] == want + e, with no value in between)
  int slot0;          // ring slot of that step; step j of the launch uses slot (slot0 + j) % ring
  int ring;
  unsigned per;       // floats between two ring slots of `in` / `out`
  unsigned steps;     // frame steps of the launch
  unsigned walk;      // steps per chunk (grid y = ceil(steps / walk))
};

// ---- the list form (LIST, on the hand-off body): the launch steps SOME streams of the batch, each by its own number of
// frames.  Wave w of the grid takes list entry w: its stream is streams[w], its frames are row w of `in` / `out`
// ([frame][n][160]: NsFlowArgs::per = n rows), and its walk is its own min(kHandoffMaxSteps, counts[w] - frame0) steps:
// one copy-in of the image, the steps, one hist_flush, one write-back.  No workgroup of the launch touches the state of
// another one's streams (the host refuses a list that names a stream twice), so nothing is handed over inside the launch:
// the list form neither polls nor publishes seq[] and never reads the abort word -- it has no spin loop -- and stream
// order between launches is all the ordering it needs.  seq[] stays what the lock-step hand-off launches left, so those
// go on before and after.  The state accesses stay sc1 and the image, the scalar row and the deferred histogram adds are
// the hand-off body's; of NsFlowArgs only `per` is read.
struct NsListArgs {
  const int32_t* streams;  // [n] stream of entry i: distinct, inside the batch (checked by the host)
  const int32_t* counts;   // [n] frames of entry i in the whole call
  int n;                   // entries (>= 1); waves past them exit behind the workgroup's barrier, as do entries with no step
  int frame0;              // frames of the call in front of this launch (`in` / `out` point at frame frame0)
};
constexpr int kListMaxSteps = 64;  // steps of an entry per launch (the host's kHandoffMaxSteps)

// The frame's new samples: 4 consecutive ones from sample `idx` of `in` (int16 frames: converted).
template <bool IO16>
__device__ __forceinline__ float4 load_frame4(const float* in, size_t idx) {
  if constexpr (IO16) {
    const short4 a = *reinterpret_cast<const short4*>(reinterpret_cast<const short*>(in) + idx);
    return make_float4((float)a.x, (float)a.y, (float)a.z, (float)a.w);
  } else {
    return *reinterpret_cast<const float4*>(in + idx);
  }
}

// the hand-off build's resident part of a stream block (dwords): everything in front of the cold rows
constexpr int kImgDwords = aspns::kOffVec + aspns::V_HOT_COUNT * aspns::kVecStride;
constexpr int kImgVec4 = kImgDwords / (64 * 4);  // 16-byte pieces per lane of a whole-image copy
static_assert(kImgDwords == 1792 && kImgDwords % (64 * 4) == 0, "the image is copied as whole 16-byte pieces per lane");
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) f32x2v lds_f32x2;
typedef __attribute__((address_space(3))) f32x4v lds_f32x4;

// One stream's state block: `uni` is a wave-uniform dword offset (a constant at every call site), `vec` the lane's
// dword offset.  Hand-off build: offsets inside the resident part address the wave's LDS image, the others memory (sc1).
template <bool FLOW>
struct StateAcc {
  float* st;
  __amdgpu_buffer_rsrc_t rs;
  lds_f32* img;
  __device__ __forceinline__ StateAcc(float* p, float* image) : st(p), img((lds_f32*)image) {
    if constexpr (FLOW) rs = __builtin_amdgcn_make_buffer_rsrc(p, 0, aspns::kStreamDwords * 4, 0x00020000);
  }
  __device__ __forceinline__ float ld1(int uni, int vec) const {
    if constexpr (FLOW) return uni < kImgDwords ? img[uni + vec] : sc1_load1(rs, vec * 4, uni * 4);
    else return st[uni + vec];
  }
  __device__ __forceinline__ float2 ld2(int uni, int vec) const {
    if constexpr (FLOW) {
      if (uni >= kImgDwords) return sc1_load2(rs, vec * 4, uni * 4);
      const f32x2v v = *reinterpret_cast<const lds_f32x2*>(img + uni + vec);
      return make_float2(v.x, v.y);
    } else {
      return *reinterpret_cast<const float2*>(st + uni + vec);
    }
  }
  __device__ __forceinline__ float4 ld4(int uni, int vec) const {
    if constexpr (FLOW) {
      if (uni >= kImgDwords) return sc1_load4(rs, vec * 4, uni * 4);
      const f32x4v v = *reinterpret_cast<const lds_f32x4*>(img + uni + vec);
      return make_float4(v.x, v.y, v.z, v.w);
    } else {
      return *reinterpret_cast<const float4*>(st + uni + vec);
    }
  }
  __device__ __forceinline__ void st1(int uni, int vec, float v) const {
    if constexpr (FLOW) {
      if (uni < kImgDwords) img[uni + vec] = v;
      else sc1_store1(rs, vec * 4, uni * 4, v);
    } else {
      st[uni + vec] = v;
    }
  }
  __device__ __forceinline__ void st2(int uni, int vec, float a, float b) const {
    if constexpr (FLOW) {
      if (uni < kImgDwords) *reinterpret_cast<lds_f32x2*>(img + uni + vec) = f32x2v{a, b};
      else sc1_store2(rs, vec * 4, uni * 4, a, b);
    } else {
      *reinterpret_cast<float2*>(st + uni + vec) = make_float2(a, b);
    }
  }
  __device__ __forceinline__ void st4(int uni, int vec, float4 x) const {
    if constexpr (FLOW) {
      if (uni < kImgDwords) *reinterpret_cast<lds_f32x4*>(img + uni + vec) = f32x4v{x.x, x.y, x.z, x.w};
      else sc1_store4(rs, vec * 4, uni * 4, x);
    } else {
      *reinterpret_cast<float4*>(st + uni + vec) = x;
    }
  }
  // the whole image: memory -> LDS (`v` are the loads of image_request, issued earlier), LDS -> memory
  __device__ __forceinline__ void image_request(int lane, float4 (&v)[kImgVec4]) const {
#pragma unroll
    for (int i = 0; i < kImgVec4; ++i) v[i] = sc1_load4(rs, lane * 16, i * 1024);
  }
  __device__ __forceinline__ void image_fill(int lane, const float4 (&v)[kImgVec4]) const {
#pragma unroll
    for (int i = 0; i < kImgVec4; ++i)
      *reinterpret_cast<lds_f32x4*>(img + i * 256 + 4 * lane) = f32x4v{v[i].x, v[i].y, v[i].z, v[i].w};
  }
  __device__ __forceinline__ void image_write_back(int lane) const {
#pragma unroll
    for (int i = 0; i < kImgVec4; ++i) {
      const f32x4v v = *reinterpret_cast<const lds_f32x4*>(img + i * 256 + 4 * lane);
      sc1_store4(rs, lane * 16, i * 1024, make_float4(v.x, v.y, v.z, v.w));
    }
  }
};

// The scalar row of a stream (ns_layout.h: 64 dwords, the per-stream scalars and the bin-128 row tails): who holds the
// master copy of slot K inside a step, behind one seam.  `sv` is the row on the lanes of one vector register.
//   * IMG = false (the plain build, and the diagnostic kernels of both builds): `sv` holds every slot; a read is a
//     v_readlane, a float write a v_cndmask under a one-lane mask;
//   * IMG = true (the product kernels of the hand-off build): `sv` holds the integer scalars (slots below S_OVERDRIVE)
//     and the three trackers' bin-128 members (lquantile and density tails, lane-resident by design); every other slot
//     -- the float scalars and the other row tails -- has its master in the wave's LDS image, where the row lies
//     anyway.  A read is an LDS read at a wave-uniform address (every lane receives the value; contiguous slots as one
//     8- or 16-byte read), a write an LDS store: neither is a vector-ALU instruction, which is what bounds the step.
//     The values arrive in vector registers -- where the plain form has them in scalar ones -- and are wave-uniform in
//     fact; the step reads each in front of its first use.  `sv`'s lanes of image-owned slots are stale inside a walk
//     and are never stored (store_owned).
// Both bodies of the step come from one text, so both use the same master for every slot.  The diagnostic kernels stay
// with IMG = false: their stamp points already hold them at 128 vector registers, and the image form needs about eight
// more at the step's widest point (profiles/README.md); what they time is the step with the plain row traffic.
template <bool IMG>
struct ScalarRow {
  lds_f32* row;  // hand-off build: the image's scalar row (a wave-uniform address)
  static constexpr int kTrk0 = aspns::S_TAIL0 + aspns::V_LQ0, kTrk1 = aspns::S_TAIL0 + aspns::V_DEN2;
  static constexpr bool in_image(int k) { return IMG && k >= aspns::S_OVERDRIVE && !(k >= kTrk0 && k <= kTrk1); }
  __device__ __forceinline__ explicit ScalarRow(float* image) : row((lds_f32*)image + aspns::kOffScalars) {}
  template <int K>
  __device__ __forceinline__ float f(float sv) const {
    if constexpr (in_image(K)) return row[K];
    else return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), K));
  }
  // slots K .. K + N - 1 (N = 2 or 4, K a multiple of N: one aligned LDS read where the image is the master)
  template <int K, int N>
  __device__ __forceinline__ void ld(float sv, float (&v)[N]) const {
    static_assert((N == 2 || N == 4) && K % N == 0 && in_image(K) == in_image(K + N - 1), "one aligned group, one master");
    if constexpr (in_image(K) && N == 2) {
      const f32x2v t = *reinterpret_cast<const lds_f32x2*>(row + K);
      v[0] = t.x; v[1] = t.y;
    } else if constexpr (in_image(K)) {
      const f32x4v t = *reinterpret_cast<const lds_f32x4*>(row + K);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), K + i));
    }
  }
  // a wave-uniform float value into slot K.  IMG: every lane that executes stores the same value to the same address
  // (the step's commit runs on lane 0 alone, the rare paths on all 64)
  template <int K>
  __device__ __forceinline__ void set(float& sv, float val) const {
    if constexpr (in_image(K)) row[K] = val;
    else sv = setlane_vgpr<K>(sv, val);
  }
  // the walk's end (hand-off build): the lanes `sv` owns go back to the image, the others are already there
  __device__ __forceinline__ void store_owned(int lane, float sv) const {
    if (!IMG || lane < aspns::S_OVERDRIVE || (lane >= kTrk0 && lane <= kTrk1)) row[lane] = sv;
  }
};

// ---- the two bodies of a frame step.  From the point where the step has read its wave-uniform scalars, the rest of
// the step exists twice, generated from ONE source text (the generic lambda `step_rest` below): the generic body, which
// serves every state a stream can be in, and the steady body, compiled under the assumption that the stream is past
// both start-up windows, that no quantile tracker publishes in this step, that the histogram window stays open and
// that gain compensation is on -- all but 6 steps in 200 and 2 in 500 of a long-running stream.  ONE predicate chooses per
// step, ns_step_is_steady(); the assumes of the steady body (ns_assume_steady) are expanded from the same list of
// conjuncts, NS_STEADY_CONJUNCTS, so the two cannot drift apart: a wrong assume is undefined behaviour, not a slow
// path.  Only wave-uniform scalars of the scalar row enter; nothing is assumed about data (the frame's energy, the
// libm fallbacks, per-lane branches).  Both bodies put every value through the same operations in the same order.
struct NsStepScalars {
  int blockInd;        // of this step: already incremented (ns_core.c:1084)
  int updates;
  int counter[3];
  int updateParsFlag;
  int mup3;            // frames left in the histogram window, before this step's decrement
  int gainmap;
};
#define NS_STEADY_CONJUNCTS(X, s)                                                                                   \
  X((s).blockInd > NS_END_STARTUP_LONG + 1)                             /* past both start-up windows */              \
  X((s).updates >= NS_END_STARTUP_LONG)                                                                              \
  X((s).counter[0] < NS_END_STARTUP_LONG - 1 && (s).counter[1] < NS_END_STARTUP_LONG - 1 &&                           \
    (s).counter[2] < NS_END_STARTUP_LONG - 1)                           /* no tracker at or next to its publish */    \
  X((s).counter[0] >= 0 && (s).counter[1] >= 0 && (s).counter[2] >= 0)                                                \
  X((s).updateParsFlag >= 1)                                                                                         \
  X((s).mup3 > 2)                                                       /* the histogram window stays open */         \
  X((s).gainmap == 1)
__device__ __forceinline__ bool ns_step_is_steady(const NsStepScalars& s) {
  bool steady = true;
#define NS_CONJ_AND(c) steady = steady && (c);
  NS_STEADY_CONJUNCTS(NS_CONJ_AND, s)
#undef NS_CONJ_AND
  return steady;
}
__device__ __forceinline__ void ns_assume_steady(const NsStepScalars& s) {
#define NS_CONJ_ASSUME(c) __builtin_assume(c);
  NS_STEADY_CONJUNCTS(NS_CONJ_ASSUME, s)
#undef NS_CONJ_ASSUME
}

// diagnostics of the DIAG instantiations (never passed by the product entry points, whose kernels have no such code)
struct NsDiagArgs {
  void* buf;  // ONE buffer, so that the step loop carries one pointer: stamps (unsigned long long) or step counts
  int mode;   // 0 = the phase stamps, 1 = the timeline (both below), 2 = step counts: [stream][2] unsigned, the steps
              // that took the steady body and the generic body, added up
};

// The frame step.  DIAG: the diagnostic stamps and the per-stream step counts exist (ns_frame1_diag_kernel); the
// product kernels (ns_frame1_kernel) are the DIAG = false instantiations, where NS_STAMP expands to nothing.
// steady_on: 0 routes every step through the generic body (AspNsBatch_SetSteady, A / B runs and tests).
// LIST: the list form of the hand-off body (NsListArgs; ns_list1_kernel); everything it changes is under `if constexpr`.
template <bool IO16, bool FLOW, bool DIAG, bool LIST = false>
__device__ __forceinline__ void ns_frame1_run(float* __restrict__ state, int32_t* __restrict__ hist_all,
                                              const NsTables* __restrict__ T, const float* __restrict__ in,
                                              float* __restrict__ out, int num_streams, int steady_on,
                                              const NsFlowArgs& fa, const NsDiagArgs& dg,
                                              [[maybe_unused]] const NsListArgs& la = NsListArgs{nullptr, nullptr, 0, 0}) {
  static_assert(!LIST || (FLOW && !DIAG), "the list form exists on the hand-off body's product kernels");
  // the diagnostic buffer (the hand-off build parks its address in a vector register pair: ns_in_vgpr)
  [[maybe_unused]] const unsigned long long diag_buf =
      DIAG ? (FLOW ? ns_in_vgpr((unsigned long long)dg.buf) : (unsigned long long)dg.buf) : 0ull;
#ifdef NS1_BUDGET
  // instruction-budget build (tools/ns_valu_budget.py, never shipped): the product code with the phase marks as
  // assembly comments and nothing else changed; a mark names the body it stands in (0 shared, 1 steady, 2 generic, 3 aside)
#define NS_STAMP(k) asm volatile("; NS_PHASE " #k " body %0" : : "n"(ns_body_tag));
  // blocks a steady step does not execute (the zero-energy exit, the walk's end, the set-up in front of the loop) are
  // bracketed: body 3 from NS_BUDGET_ASIDE to the NS_BUDGET_BACK(k) that names the phase and body it returns to
#define NS_BUDGET_ASIDE() asm volatile("; NS_PHASE 99 body 3");
#define NS_BUDGET_BACK(k) asm volatile("; NS_PHASE " #k " body %0" : : "n"(ns_body_tag));
#else
  // diagnostic stamps.  stamp_mode 0: the 16 phase stamps
  // (shader clock) of workgroup 0's first wave (hand-off build: of the middle of the launch, x = grid / 2,
  // step = steps / 2, plus a 17th at that step's end: once its stores have drained where it is its walk's last).  stamp_mode 1 ("timeline"): every workgroup's first
  // wave records the 100 MHz real-time counter at its start, after its first loads, before its last
  // stores and at its end (4 values per workgroup) -- the launch-level picture.
  // One wave-uniform word decides: 0 = this wave takes no stamp, 1 = the timeline, 2 + j = the phase stamps, in step j
  // of the launch (the plain build: j = 0).  The DIAG kernels must hold the register budget of the product kernels
  // (tests/test_ns_steady_host.py), so a stamp point keeps nothing else alive: the buffer comes from `dg` where it is
  // written.
  [[maybe_unused]] unsigned stamp_sel = 0;
  if constexpr (DIAG) {
    if (dg.buf != nullptr && dg.mode != 2 && threadIdx.x < 64) {
      if (dg.mode == 1) stamp_sel = 1u;
      else if (FLOW ? blockIdx.x == gridDim.x / 2 : blockIdx.x == 0) stamp_sel = 2u + (FLOW ? fa.steps / 2 : 0u);
    }
  }
  // (a scalar branch only: every lane of the stamping wave stores the same value to the same address)
#define NS_STAMP(k)                                                                            \
  if constexpr (DIAG) {                                                                        \
    const unsigned stamp_sel_ = __builtin_amdgcn_readfirstlane(stamp_sel);                     \
    if (stamp_sel_ != 0) {                                                                     \
      __builtin_amdgcn_sched_barrier(0);                                                       \
      unsigned long long* const stamps_ = reinterpret_cast<unsigned long long*>(diag_buf);     \
      if (stamp_sel_ == 1u) {                                                                  \
        if ((k) == 0 || (k) == 1 || (k) == 14 || (k) == 15)                                    \
          stamps_[blockIdx.x * 4 + ((k) == 0 ? 0 : (k) == 1 ? 1 : (k) == 14 ? 2 : 3)] =       \
              __builtin_amdgcn_s_memrealtime() | ((k) == 0 ? ns_cu_tag() << 48 : 0ull);       \
      } else if (stamp_sel_ == 2u + flow_j) {                                                  \
        stamps_[k] = __builtin_amdgcn_s_memtime();                                             \
      }                                                                                        \
      __builtin_amdgcn_sched_barrier(0);                                                       \
    }                                                                                          \
  }
#define NS_BUDGET_ASIDE()
#define NS_BUDGET_BACK(k)
#endif
  // the hand-off build's chunk of the launch: steps flow_j .. flow_end - 1; step flow_j uses ring slot flow_slot
  unsigned flow_j = 0, flow_end = 1, flow_slot = 0;
  // DIAG: the steps of this walk that took the steady body (low half) and the generic one (high half: a walk has at
  // most 64 steps), added to the stream's two counts when the wave is done
  [[maybe_unused]] unsigned diag_steps = 0;
  [[maybe_unused]] constexpr int ns_body_tag = 0;  // (budget build: the marks outside the two bodies)
  if constexpr (LIST) {
    // the wave's walk is steps 0 .. (its count) - 1 of the launch's slice, frame j in slot j: set where the entry is read
  } else if constexpr (FLOW) {
    flow_j = blockIdx.y * fa.walk;
    flow_end = flow_j + fa.walk < fa.steps ? flow_j + fa.walk : fa.steps;
    flow_slot = ((unsigned)fa.slot0 + flow_j) % (unsigned)fa.ring;
  } else {
    NS_STAMP(0)
  }
  __shared__ __align__(16) float2 lds[4][130];  // 128 elements + the slot lane 0 reads past them (ns_pair_fft.h)
  // per-lane twiddles of the three passes (3 x 64 x 4), real-split factors (32 x 4 x 2) and the
  // window, staged in LDS once per workgroup behind the (first step's) state loads
  __shared__ __align__(16) float tabs[3 * 64 * 4 + 32 * 4 * 2];
  __shared__ __align__(16) float wins[kAnal];
  __shared__ __align__(16) double exp2s[64];     // 2^(j/64) of the lean exp / tanh
  __shared__ __align__(16) double2 logts[128];   // {1/c, log c} of the table-driven log
  // hand-off build: each wave's image of its stream's resident state block (the plain build has no use: no allocation)
  __shared__ __align__(16) float imgs[FLOW ? 4 : 1][FLOW ? kImgDwords : 4];
  // hand-off build, product kernels: the histogram features of the walk's steady steps that are not yet counted
  // (hist_flush below): kPendSteps slots of three floats per wave, -1 in a slot that holds nothing
  constexpr bool DEFER = FLOW && !DIAG;
  constexpr int kPendSteps = 8, kPendLanes = 3 * kPendSteps;
  __shared__ __align__(16) float pends[DEFER ? 4 : 1][DEFER ? kPendLanes : 1];
  const int tid = threadIdx.x;
  // ---- prologue: every load of the first phase is issued before the first wait (table pieces
  // first: loads return in order, the LDS staging waits for them only)
  const float4* tab_src = tid < 192 ? reinterpret_cast<const float4*>(&T->tw[0][0][0]) + tid
                                    : reinterpret_cast<const float4*>(&T->spl[0][0][0]) + (tid - 192);
  const float4 tab_v = *tab_src;
  const float4 win_v = reinterpret_cast<const float4*>(T->window)[tid & 63];
  const double exp2_v = T->exp2_64[tid & 63];
  const double2 logt_v = reinterpret_cast<const double2*>(T->logtab)[tid & 127];
  const int lane = tid & 63;
  const int diagbits = T->diag[lane];
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  float2* tile = lds[wv];
  const int lam = lane >> 1, h = lane & 1;
  const int g = lam >> 4, q = lam & 15;
  const int binA = q + 64 * g + 16 * h;  // slot 0; slot 1 = binA + 32; slot 2 = bin 128
  const uint32_t gmask = g ? 0x80000000u : 0u;
  const int stream_raw = blockIdx.x * 4 + wv;
  bool wave_live = stream_raw < num_streams;
  // `stream` is the wave's row of a frame of `in` / `out` and, but for the list form, the index of its state block
  // (list form: the wave's list entry; the kernel passes the list's length as num_streams)
  const int stream = wave_live ? stream_raw : num_streams - 1;  // clamped for the loads
  [[maybe_unused]] int list_stream = 0;
  if constexpr (LIST) {
    // the entry's words: wave-uniform scalar loads of what the host wrote before the launch
    const int left = la.counts[stream] - la.frame0;
    flow_end = left < 0 ? 0u : (left > kListMaxSteps ? (unsigned)kListMaxSteps : (unsigned)left);
    wave_live = wave_live && flow_end != 0u;
    list_stream = la.streams[stream];
  }
  const int state_ix = LIST ? list_stream : stream;
  float* __restrict__ st = state + (size_t)state_ix * kStreamDwords;
  int32_t* __restrict__ hist = hist_all + (size_t)state_ix * kHistDwords;
  const StateAcc<FLOW> sa(st, FLOW ? imgs[wv] : nullptr);
  float* outj = out;  // this step's frame of `out` (hand-off build: its ring slot)
  auto diag_flush_steps = [&]() __attribute__((always_inline)) {
    if constexpr (DIAG) {
      unsigned* const counts = reinterpret_cast<unsigned*>(diag_buf);
      if (dg.mode == 2 && ns_cold(lane) == 0) {
        atomicAdd(counts + 2 * stream, diag_steps & 0xffffu);
        atomicAdd(counts + 2 * stream + 1, diag_steps >> 16);
      }
    }
  };

  // ---- the histogram increments of a walk, once per walk (DEFER).  Past start-up every step adds one count to each
  // of the three feature histograms (FeatureParameterExtraction(self, 0), ns_core.c:309-334); the counts commute and
  // are read only where a window closes, which is a generic step.  A step of the steady body therefore only RECORDS
  // its three feature values, in slot (step of the walk) % kPendSteps of the wave's `pends`; hist_flush() does the bin
  // arithmetic and the no-return atomic adds for every recorded step at once, slot i's feature f on lane 3 i + f,
  // through the operations of the per-step form, and empties the slots.  It runs at the walk's end in front of the
  // write-back and the drain (nothing is pending when the walk is published), in front of everything a generic step
  // does with the histograms, and in front of every record past the walk's first kPendSteps steps (a longer walk reuses
  // its slots).  A step that adds nothing now records nothing: the zero-energy exit, and the generic body, which keeps
  // the per-step form.  (Owner and validity of the slots: DESIGN.md section 4.)
  lds_f32* const pend = (lds_f32*)pends[DEFER ? wv : 0];
  auto hist_flush = [&]() __attribute__((always_inline)) {
    if constexpr (DEFER) {
      const int lane_c = ns_cold(lane);
      lds_sync1();
      if (lane_c < kPendLanes) {
        const float fv = pend[lane_c];
        pend[lane_c] = -1.f;
        const int f = lane_c % 3;  // 0: LRT, 1: spectral flatness, 2: spectral difference
        const float bw = f == 1 ? 0.05f : 0.1f, rbw = f == 1 ? 1.0f / 0.05f : 1.0f / 0.1f;
        const float lim = f == 1 ? kHist * 0.05f : kHist * 0.1f;
        if ((fv < lim) && (fv >= 0.0f))
          atomicAdd(&hist[f * kHistStride + (int)div_by_uniform(fv, bw, rbw)], 1);  // agent scope (sc1)
      }
      lds_sync1();
    }
  };

  // ---- scalars: lane k holds scalar k (wave-uniform values, read with v_readlane); the hand-off build keeps the
  // float scalars and most row tails in the image instead (ScalarRow)
  float sv;
  constexpr bool ROW_IMG = FLOW && !DIAG;  // who holds the float scalars and the row tails (ScalarRow)
  const ScalarRow<ROW_IMG> srow(imgs[FLOW ? wv : 0]);
#define SC_I(k) __builtin_amdgcn_readlane(__float_as_int(sv), (k))
#define SC_F(k) srow.template f<(k)>(sv)
#define SC_SET_I(k, val) sv = writelane_bits<(k)>(sv, (int)(val))
#define SC_SET_F(k, val) srow.template set<(k)>(sv, (val))
  // (the steady body commits its integer scalars as two carry adds on `sv` under constant lane masks, addlanes_bits:
  // blockInd and the three counters + 1, mup3 - 1, updates and updateParsFlag unchanged -- a step of the steady body
  // resets no counter and closes no window)
  static_assert(S_COUNTER1 == S_COUNTER0 + 1 && S_COUNTER2 == S_COUNTER0 + 2, "the three counters: consecutive lanes");
  // ---- sliding analysis buffer [96 carried | 160 new]: lane L owns samples 4L .. 4L+3
  float4 s4;
  // syntBuf[0..95]: the lane's output samples 2E, 2E+1 that still carry overlap are those of
  // slot 0 when g == 0 (2q + 32h) and of slot 1 when g == 0 and h == 0 (2q + 64); every lane
  // loads (no branch), the overlap-add uses the owners' values only
  float2 carryA, carryB;
  // hand-off build: the new samples of the frame in ring slot `slot` (lanes 24..63; the others load lane 24's and
  // drop them).  They do not depend on the hand-off: requested ahead of the state -- for the chunk's first step
  // before the poll, for the others before the previous step's last stores.
  float4 s4in = make_float4(0.f, 0.f, 0.f, 0.f);
  const size_t frame_uni = (size_t)stream * kBlockL;  // the stream's samples inside a frame (wave-uniform)
  auto flow_load_in = [&](unsigned slot) __attribute__((always_inline)) {
    const int lane_c = ns_cold(lane);
    const unsigned frame_lane = 4u * (unsigned)((lane_c < 24 ? 24 : lane_c) - 24);
    const float* base = IO16 ? reinterpret_cast<const float*>(reinterpret_cast<const short*>(in + (size_t)slot * fa.per) + frame_uni)
                             : in + (size_t)slot * fa.per + frame_uni;
    s4in = load_frame4<IO16>(base, frame_lane);
  };
  // hand-off build: the first state reads of step flow_j, from the image (the scalar row is read once per walk and
  // stays in `sv` between the walk's steps)
  // (head_c: the budget build's body tag of this copy of the head -- 0 where a step that goes on executes it, 3 for
  // the copy in front of the loop and the one behind the zero-energy exit)
  auto flow_head = [&](auto head_c) __attribute__((always_inline)) {
    [[maybe_unused]] constexpr int ns_body_tag = decltype(head_c)::value;
    NS_STAMP(0)
    outj = out + (size_t)flow_slot * fa.per;
    const int lane_c = ns_cold(lane);
    // each lane takes its own source, the carried 96 (lanes 0..23) or the new 160, into the same registers: the read of
    // the carried samples runs on its lanes alone, over what they loaded of the new frame and dropped
    s4 = s4in;
    if (lane_c < 24) s4 = sa.ld4(kOffAnaHist, 4 * lane_c);
    const int q2_c = lane_c & 30;  // 2 q
    carryA = sa.ld2(kOffSynt, q2_c + 32 * (lane_c & 1));
    carryB = sa.ld2(kOffSynt, q2_c + 64);
  };
  [[maybe_unused]] float4 img_v[FLOW ? kImgVec4 : 1];
  if constexpr (FLOW) {
    // (list form: an entry without a step reads no frame, and there is nothing to wait for: NsListArgs)
    if (!LIST || wave_live) flow_load_in(flow_slot);
    if constexpr (!LIST)
      if (wave_live) wave_live = handoff_wait(fa.hand, fa.want + flow_j, stream, lane);
    if (wave_live) sa.image_request(lane, img_v);  // the copy-in: in flight behind the table staging
  } else {
    sv = st[kOffScalars + lane];
    float* hbuf = st + kOffAnaHist;
    if (!IO16) {
      const float* src = lane < 24 ? hbuf + 4 * lane : in + (size_t)stream * kBlockL + 4 * (lane - 24);
      s4 = *reinterpret_cast<const float4*>(src);
    } else {
      const int lh = lane < 24 ? lane : 23, li = lane < 24 ? 24 : lane;
      const float4 ha = *reinterpret_cast<const float4*>(hbuf + 4 * lh);
      const short* in16 = reinterpret_cast<const short*>(in) + (size_t)stream * kBlockL + 4 * (li - 24);
      const short4 a = *reinterpret_cast<const short4*>(in16);
      const bool hsel = lane < 24;
      s4.x = hsel ? ha.x : (float)a.x;
      s4.y = hsel ? ha.y : (float)a.y;
      s4.z = hsel ? ha.z : (float)a.z;
      s4.w = hsel ? ha.w : (float)a.w;
    }
    carryA = *reinterpret_cast<const float2*>(st + kOffSynt + 2 * q + 32 * h);
    carryB = *reinterpret_cast<const float2*>(st + kOffSynt + 2 * q + 64);
  }

  // ---- table staging (the loads above are in flight behind it)
  reinterpret_cast<float4*>(tabs)[tid] = tab_v;
  if (tid < 64) exp2s[tid] = exp2_v;
  if (tid < 128) logts[tid] = logt_v;
  if (tid >= 192) reinterpret_cast<float4*>(wins)[tid - 192] = win_v;
  if constexpr (FLOW) {
    if (wave_live) sa.image_fill(lane, img_v);
  }
  if constexpr (DEFER) {
    if (lane < kPendLanes) pends[wv][lane] = -1.f;
  }
  __syncthreads();
  if (!wave_live) return;
  if constexpr (FLOW) {
    sv = sa.ld1(kOffScalars, lane);
    flow_head(std::integral_constant<int, 3>{});
  }
  const float* tws = tabs;
  const float* spls = tabs + 3 * 64 * 4;
  const PairFftLane fl = pair_fft_lane(lane, diagbits);

#define LOADV(dst, f)                                                                          \
  {                                                                                            \
    const float2 v2_ = sa.ld2(kOffVec + (f)*kVecStride, 2 * lane);                             \
    dst[0] = v2_.x; dst[1] = v2_.y;                                                            \
  }
#define LOADT(dst, f) dst[2] = SC_F(S_TAIL0 + (f));
#define LOAD3(dst, f) LOADV(dst, f) LOADT(dst, f)
#define STORE3(f, srcv)                                                                        \
  {                                                                                            \
    sa.st2(kOffVec + (f)*kVecStride, 2 * lane, srcv[0], srcv[1]);                              \
    SC_SET_F(S_TAIL0 + (f), srcv[2]);                                                          \
  }
  // the same for the five rows every step writes: the hand-off build stores their tails with the step's float scalars,
  // on one lane (commit_floats)
#define STORE3_HOT(f, srcv)                                                                    \
  {                                                                                            \
    sa.st2(kOffVec + (f)*kVecStride, 2 * lane, srcv[0], srcv[1]);                              \
    if constexpr (!ROW_IMG) SC_SET_F(S_TAIL0 + (f), srcv[2]);                                  \
  }
  // the frame of the chunk's next step is requested while this step still has its inverse transform ahead
#define NS_NEXT_FRAME()                                                                        \
  if constexpr (FLOW) {                                                                        \
    if constexpr (LIST) flow_slot = flow_slot + 1u; /* (frame j + 1 of the slice; requested only below the count) */ \
    else flow_slot = flow_slot + 1u == (unsigned)fa.ring ? 0u : flow_slot + 1u;                \
    if (flow_j + 1u < flow_end) flow_load_in(flow_slot);                                       \
  }
  // the step is done for this stream.  Hand-off build: after the walk's last step the wave writes its image back,
  // drains every store it has issued and publishes the walk; otherwise it goes on to its next step on the image (the
  // wave-level fence orders this step's image writes, other lanes' too, in front of the next step's reads)
#define NS_STREAM_DONE(head_tag)                                                               \
  if constexpr (FLOW) {                                                                        \
    [[maybe_unused]] constexpr int ns_body_tag = head_tag; /* (budget build: where this copy stands) */ \
    const bool walk_done_ = flow_j + 1u >= flow_end;                                           \
    if (walk_done_) {                                                                          \
      NS_BUDGET_ASIDE()                                                                        \
      const int lane_w_ = ns_cold(lane);                                                       \
      srow.store_owned(lane_w_, sv);                                                           \
      hist_flush(); /* (orders the image's LDS writes in front of the write-back too) */      \
      if constexpr (!DEFER) lds_sync1();                                                       \
      sa.image_write_back(lane_w_);                                                            \
      handoff_drain();                                                                         \
    }                                                                                          \
    NS_STAMP(16)                                                                               \
    if (walk_done_) {                                                                          \
      NS_BUDGET_ASIDE()                                                                        \
      diag_flush_steps();                                                                      \
      if (!LIST && lane == 0) handoff_publish(fa.hand.seq + stream, fa.want + flow_j);         \
      return;                                                                                  \
    }                                                                                          \
    ++flow_j;                                                                                  \
    lds_sync1();                                                                               \
    NS_BUDGET_BACK(16)                                                                         \
    flow_head(std::integral_constant<int, head_tag>{});                                        \
    continue;                                                                                  \
  } else {                                                                                     \
    diag_flush_steps();                                                                        \
    return;                                                                                    \
  }

  // ---- carried across the steps of a walk (hand-off build).  ComputeSnr and the Wiener gain of step t + 1 both want
  // magnPrev / (noisePrev + 0.0001f) * smooth (ns_core.c:576-577, 993-994), and step t had exactly that quotient in
  // registers: its phase 11 forms gq1 = magn / (noise + 0.0001f) and then stores that magn, noise and gain as the three
  // rows (ns_core.c:1304-1310).  Same operands, same operations, same bits: prevStsa(t + 1) == gq1(t) * gainv(t).  The
  // step that produced the product owns it; carry_ok says that one did in THIS walk (wave-uniform, tested with a scalar
  // branch).  A walk starts without it and reads the rows, whoever wrote them last -- the previous walk, the host,
  // InitStream, an import; the zero-energy exit touches neither the rows nor the carry (ns_core.c:1239-1264).
  constexpr bool CARRY = FLOW;
  [[maybe_unused]] f32x2 carry_stsa = {0.f, 0.f};  // the lane's two bins
  [[maybe_unused]] float carry_stsa_tail = 0.f;    // bin 128
  [[maybe_unused]] bool carry_ok = false;
  // The refined reciprocal of quant + 0.0001f (the first part of ComputeSnr's division, fdiv2_rcp / fdiv_rcp): in the
  // steady body the noise estimate IS the stored quantile, which only a publish changes, and a publish is a generic
  // step.  A steady step owns it; rcpq_ok says that the previous live step of THIS walk was one (a generic step clears
  // it, a walk starts without it, the zero-energy exit touches neither the quantile nor the carry).
  // (the product kernels only: the diagnostic hand-off kernel has no registers for it, as for ROW_IMG)
  constexpr bool RCPQ = FLOW && !DIAG;
  [[maybe_unused]] f32x2 rcpq = {0.f, 0.f};
  [[maybe_unused]] float rcpq_tail = 0.f;
  [[maybe_unused]] bool rcpq_ok = false;
  for (;;) {  // the steps of the chunk (one pass in the plain build); no barrier inside: each wave owns its LDS tile
    NS_BUDGET_BACK(0)
    // state rows are requested in two groups, just ahead of their use (requesting all of them before
    // the first wait measured slower: every wave of a launch starts at once, and a bigger
    // start-of-kernel burst makes every wave wait longer)
    float LQ[3][NS3], DEN[3][NS3], quant[NS3];
    float smooth[NS3], noisePrev[NS3], magnPrevA[NS3], logLrt[NS3], avgPause[NS3];


    const float4 w4 = *reinterpret_cast<const float4*>(wins + 4 * lane);
    const float wx0 = w4.x * s4.x, wx1 = w4.y * s4.y, wx2 = w4.z * s4.z, wx3 = w4.w * s4.w;
    // Windowing + Energy (ns_core.c:969-978, 951-960)
    float epart = wx0 * wx0;
    epart += wx1 * wx1;
    epart += wx2 * wx2;
    epart += wx3 * wx3;
    const float energy1 = wave_sum_bcast(epart);

    // the carried 96 samples of the next frame are this frame's last 96
    {
      const int lane_c = ns_cold(lane);
      if (lane_c >= 40) sa.st4(kOffAnaHist, 4 * (lane_c - 40), s4);
    }

    if (energy1 == 0.0f) {
      NS_BUDGET_ASIDE()
      // Analyze: nothing but the buffer slide (ns_core.c:1072-1082); Process: emit the synthesis
      // tail and clear it (ns_core.c:1239-1264)
      float* y = IO16 ? reinterpret_cast<float*>(reinterpret_cast<short*>(outj) + (size_t)stream * kBlockL)
                      : outj + (size_t)stream * kBlockL;
      NS_NEXT_FRAME()
      const int lane_c = ns_cold(lane);
      float2 o01 = make_float2(0.f, 0.f);
      if (lane_c < 48) o01 = sa.ld2(kOffSynt, 2 * lane_c);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      store2p<IO16>(y, 2 * lane_c, sat16p(o01.x), sat16p(o01.y));
      if (lane_c < 16) store2p<IO16>(y, 128 + 2 * lane_c, 0.f, 0.f);
      if (lane_c < 48) sa.st2(kOffSynt, 2 * lane_c, 0.f, 0.f);
      NS_STREAM_DONE(3)
    }
    NS_BUDGET_BACK(0)

    // the tracker rows are requested once the frame's samples are in; they are used after the
    // transform, the magnitudes and the logarithms
    LOADV(LQ[0], V_LQ0) LOADV(LQ[1], V_LQ1) LOADV(LQ[2], V_LQ2)
    LOADV(DEN[0], V_DEN0) LOADV(DEN[1], V_DEN1) LOADV(DEN[2], V_DEN2)
    LOADV(quant, V_QUANT)  // (the trackers' bin-128 members stay on their lanes of the scalar row: phase 4)
    NS_STAMP(1)
    // ---- forward FFT (ns_core.c:886-911)
    *reinterpret_cast<float4*>(&tile[2 * lane]) = make_float4(wx0, wx1, wx2, wx3);
    lds_sync1();
    f32x2 er, ei;  // the lane's two bins {slot 0, slot 1}: real parts, imaginary parts
    {
      f32x2 ea, eb;
      cft128_passes1(tile, tws, fl, lane, ea, eb);
      radix2_tail1(ea, eb, gmask, false, er, ei);
    }
    real_split1(tile, spls, lane, er, ei, false);

    NS_STAMP(2)
    // second group of state rows (latency hides under magnitude / log / trackers)
    // (the hand-off build reads magnPrev and smooth in phase 6, and only in a step that has no carried product)
    if constexpr (!CARRY) LOADV(magnPrevA, V_MAGNPREV_A)
    LOADV(logLrt, V_LOGLRT) LOADV(avgPause, V_AVGPAUSE)
    if constexpr (!CARRY) LOADV(smooth, V_SMOOTH)
    LOADV(noisePrev, V_NOISEPREV)
    // (their bin-128 members are read from the scalar row where they are first used: wave-uniform values that the
    // hand-off build holds in vector registers, which the transform's end has none to spare of)

    float re[NS3], im[NS3], magn[NS3];
    re[0] = er.x;
    im[0] = ei.x;
    re[1] = er.y;
    im[1] = ei.y;
    re[2] = lane_bcast(ei.x, 0);  // R128 sits in the imaginary slot of element 0 (lane 0, slot 0)
    im[2] = 0.f;
    if (lane == 0) im[0] = 0.f;
    {
      float m2[2] = {re[0] * re[0] + im[0] * im[0], re[1] * re[1] + im[1] * im[1]}, rt[2];
      fsqrt_n_wave<2>(m2, rt);
      magn[0] = rt[0] + 1.f;
      magn[1] = rt[1] + 1.f;
    }
    if (lane == 0) magn[0] = fabsf(re[0]) + 1.f;
    magn[2] = fabsf(re[2]) + 1.f;

    // sum over the 129 bins of a per-bin quantity: the lane's two owned bins, the wave64 butterfly over the
    // 64 partials, then bin 128 (association ASP_NS_REDUCE_TREE64P of oracle/ns_oracle.c)
#define SUM3(v) (wave_sum_bcast(v[0] + v[1]) + v[2])

    // the wave-uniform scalars that decide which body serves the step, and the decision
    NsStepScalars ss;
    ss.blockInd = SC_I(S_BLOCKIND) + 1;  // ns_core.c:1084
    ss.updates = SC_I(S_UPDATES);
    ss.counter[0] = SC_I(S_COUNTER0);
    ss.counter[1] = SC_I(S_COUNTER1);
    ss.counter[2] = SC_I(S_COUNTER2);
    ss.updateParsFlag = SC_I(S_MUP0);
    ss.mup3 = SC_I(S_MUP3);
    ss.gainmap = SC_I(S_GAINMAP);
    const bool step_steady = steady_on != 0 && ns_step_is_steady(ss);
    // the trackers' counter terms {n - 1, n, 1 / n} as floats (n - 1 = counter[s] = 0 .. 200): functions of an integer in
    // a scalar register, read from NsTables::cnt_terms with wave-uniform scalar loads and used in phase 4.  Each body
    // requests them as its first act -- the earliest place behind the counters; requested in front of the split into the
    // two bodies, every ns_frame1 kernel spilled vector registers (profiles/README.md).  One dword per load: the
    // compiler turns a wider read of an entry into a vector load.  (A valid state keeps its counters in 0 .. 200,
    // ns_core.c:262-272; the index is held inside the table whatever an imported state carries.)
    static_assert(kCntTerms == NS_END_STARTUP_LONG + 1, "one entry per counter value");
    float cterm[3][3];
    auto load_cterms = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        typedef const __attribute__((address_space(4))) float cfloat_k;
        const unsigned n = (unsigned)ss.counter[s] < (unsigned)NS_END_STARTUP_LONG ? (unsigned)ss.counter[s]
                                                                                   : (unsigned)NS_END_STARTUP_LONG;
#pragma unroll
        for (int j = 0; j < 3; ++j) cterm[s][j] = *(cfloat_k*)(&T->cnt_terms[n][j]);
      }
    };
    // ---- the rest of the step, up to the commit of its scalars: ONE text, instantiated as the steady body
    // (steady_c = std::true_type: under the assumes of ns_assume_steady) and as the generic one.  It is a lambda: a
    // `return` inside would leave the lambda and not the kernel, and `continue` is not available; the step ends
    // behind the two calls below, in NS_STREAM_DONE.
    auto step_rest = [&](auto steady_c) __attribute__((always_inline)) {
      constexpr bool STEADY = decltype(steady_c)::value;
      [[maybe_unused]] constexpr int ns_body_tag = STEADY ? 1 : 2;
      if constexpr (STEADY) ns_assume_steady(ss);
      if constexpr (DIAG) diag_steps += STEADY ? 1u : 0x10000u;
      load_cterms();
      const int blockInd = ss.blockInd;
      float priorSpeechProb;  // (read in front of the tanh of phase 9; overdrive and denoiseBound: phase 11)
      const int gainmap = ss.gainmap;

      float noise[NS3], prevStsa[NS3];
      const int updateParsFlag = ss.updateParsFlag;
      int updates = ss.updates;
      int counter[3] = {ss.counter[0], ss.counter[1], ss.counter[2]};

      // Bin 128 of ComputeSnr (ns_core.c:566-588; the lane's two bins: phase 6), every value through the operations of
      // the per-bin loop.  noise2: bin 128 of the noise estimate.
      float snrLocPost[NS3], snrLocPrior[NS3];
      auto snr_tail = [&](float noise2) __attribute__((always_inline)) {
        const float d2t = noise2 + 0.0001f;
        float r2t;
        if (RCPQ && STEADY && rcpq_ok) {
          r2t = rcpq_tail;
        } else {
          r2t = fdiv_rcp(d2t);
          // (a marked value: the compiler turns an unmarked short else-path into both paths and a select)
          if constexpr (RCPQ && STEADY) asm volatile("; the quantile's reciprocal, bin 128" : "+v"(r2t));
        }
        if constexpr (RCPQ && STEADY) rcpq_tail = r2t;
        const float q2t = fdiv_quot(magn[2], d2t, r2t);  // used where magn > noise
        float previousEstimateStsa;
        if (CARRY && carry_ok) {
          previousEstimateStsa = carry_stsa_tail;
        } else {
          const float q1t = fdiv(magnPrevA[2], noisePrev[2] + 0.0001f);
          previousEstimateStsa = q1t * smooth[2];
        }
        prevStsa[2] = previousEstimateStsa;
        snrLocPost[2] = 0.f;
        if (magn[2] > noise2) snrLocPost[2] = q2t - 1.f;
        snrLocPrior[2] = NS_DD_PR_SNR * previousEstimateStsa + (1.f - NS_DD_PR_SNR) * snrLocPost[2];
      };
      auto load_snr_tails = [&]() __attribute__((always_inline)) {
        static_assert(V_SMOOTH == V_QUANT + 1 && V_MAGNPREV_A == V_NOISEPREV + 1, "row tails read as pairs");
        float t2[2], u2[2];
        srow.template ld<S_TAIL0 + V_QUANT, 2>(sv, t2);
        srow.template ld<S_TAIL0 + V_NOISEPREV, 2>(sv, u2);
        quant[2] = t2[0]; smooth[2] = t2[1];
        noisePrev[2] = u2[0]; magnPrevA[2] = u2[1];
      };
      // The step's two logarithms of bin 128 -- log magn (here) and log(1 + 2 snrLocPrior) (phase 8) -- share ONE third
      // slot in the steady body: no tracker publishes and the start-up model is off, so the noise estimate of bin 128 is
      // the stored quantile and the second argument needs only magn[2] and loaded state.  It is computed ahead, goes on
      // lane 1 of this call's third slot beside magn[2] on the other lanes, and both results come back by broadcast; the
      // second call then serves the lane's two bins only.  The generic body keeps two three-slot calls.
      float lmagn[NS3];
      [[maybe_unused]] float lt1_tail = 0.f;
      if constexpr (STEADY) {
        load_snr_tails();
        snr_tail(quant[2]);
        const float xs[NS3] = {magn[0], magn[1], lane == 1 ? 1.f + 2.f * snrLocPrior[2] : magn[2]};
        log_f32_via_tab_n_wave<NS3>(xs, lmagn, logts);
        lt1_tail = lane_bcast(lmagn[2], 1);
        lmagn[2] = lane_bcast(lmagn[2], 0);
      } else {
        log_f32_via_tab_n_wave<NS3>(magn, lmagn, logts);
      }
      LOADT(avgPause, V_AVGPAUSE)

      NS_STAMP(3)
      // the four cross-bin sums that need only this frame's spectrum and the loaded rows, reduced side by
      // side: signal energy (ns_core.c:1089-1103), sum of magnitudes, the flatness numerator (bins 1..128,
      // :535-541) and the mean of magnAvgPause (:603-607)
      float signalEnergy, sumMagn, flatNum, avgPauseMean;
      {
        float p_se = (re[0] * re[0] + im[0] * im[0]) + (re[1] * re[1] + im[1] * im[1]);
        float p_sm = magn[0] + magn[1];
        float p_fl = lane == 0 ? lmagn[1] : lmagn[0] + lmagn[1];
        float p_ap = avgPause[0] + avgPause[1];
        wave_sums_bcast(p_se, p_sm, p_fl, p_ap);
        signalEnergy = p_se + (re[2] * re[2] + im[2] * im[2]);
        sumMagn = p_sm + magn[2];
        flatNum = p_fl + lmagn[2];
        avgPauseMean = p_ap + avgPause[2];
        signalEnergy = DIV129(signalEnergy);
      }

      NS_STAMP(4)
      // (generic body: the row tails ComputeSnr wants, phase 6, requested here: the trackers' work covers the LDS round trip)
      if constexpr (!STEADY) load_snr_tails();
      // ---- NoiseEstimation (ns_core.c:217-285)
      if (updates < NS_END_STARTUP_LONG) updates++;
      bool quant_new = false;
      // Bin 128 of the three trackers: three independent chains with one formula, evaluated ONCE with tracker s on
      // lane 48 + s -- where its lquantile tail already sits in the scalar row; its density tail, three lanes up in
      // the same DPP row, comes down by one row shift, and n - 1 / n / 1 / n are put on the three lanes from the
      // trackers' table terms (cterm).  Every value goes through the operations of its own wave-uniform pass; the
      // other lanes compute on whatever the row holds and are dropped by the masked merge.
      constexpr int kLqLane = S_TAIL0 + V_LQ0, kDenLane = S_TAIL0 + V_DEN0;
      static_assert(V_LQ1 == V_LQ0 + 1 && V_LQ2 == V_LQ0 + 2 && V_DEN1 == V_DEN0 + 1 && V_DEN2 == V_DEN0 + 2 &&
                    kDenLane == kLqLane + 3 && kLqLane / 16 == (kDenLane + 2) / 16,
                    "the tracker tails: three + three consecutive lanes of one DPP row");
      float lqT = sv, denT = dpp_move<0x103>(sv);  // row_shl:3: lane L reads lane L + 3
      {
#define NS_LANES3_F(j) __int_as_float(lanes3_bits<kLqLane>(__float_as_int(cterm[0][j]), __float_as_int(cterm[1][j]), \
                                                           __float_as_int(cterm[2][j])))
        const float cntv = NS_LANES3_F(0), cnt1v = NS_LANES3_F(1), rcnt1v = NS_LANES3_F(2);  // rcnt1 == 1.f / cnt1
#undef NS_LANES3_F
        tracker_step1_c(lqT, denT, lmagn[2], cntv, cnt1v, rcnt1v);
      }
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        {
          const float cnt = cterm[s][0], cnt1 = cterm[s][1], rcnt1 = cterm[s][2];
          f32x2 lq = {LQ[s][0], LQ[s][1]}, den = {DEN[s][0], DEN[s][1]};
          tracker_step2_c(lq, den, f32x2{lmagn[0], lmagn[1]}, cnt, cnt1, rcnt1);
          LQ[s][0] = lq.x; LQ[s][1] = lq.y;
          DEN[s][0] = den.x; DEN[s][1] = den.y;
        }
        if (counter[s] >= NS_END_STARTUP_LONG) {
          counter[s] = 0;
          if (updates >= NS_END_STARTUP_LONG) {
            LQ[s][2] = lane_bcast(lqT, kLqLane + s);  // the publish wants the tail wave-uniform
            exp_f32_via_f64_n_wave<NS3>(LQ[s], quant, exp2s);
            quant_new = true;
          }
        }
        counter[s]++;
      }
      if (updates < NS_END_STARTUP_LONG) {
        LQ[2][2] = lane_bcast(lqT, kLqLane + 2);
        exp_f32_via_f64_n_wave<NS3>(LQ[2], quant, exp2s);
        quant_new = true;
      }
#pragma unroll
      for (int k = 0; k < NS3; ++k) noise[k] = quant[k];
#pragma unroll
      for (int s = 0; s < 3; ++s) sa.st2(kOffVec + (V_LQ0 + s) * kVecStride, 2 * lane, LQ[s][0], LQ[s][1]);
#pragma unroll
      for (int s = 0; s < 3; ++s) sa.st2(kOffVec + (V_DEN0 + s) * kVecStride, 2 * lane, DEN[s][0], DEN[s][1]);
      sv = mergelanes_vgpr<(7ull << kLqLane)>(sv, lqT);
      sv = mergelanes_vgpr<(7ull << kDenLane)>(sv, dpp_move<0x113>(denT));  // row_shr:3: lane L reads lane L - 3
      // the published quantile changes once in ~67 frames past start-up (a tracker publishes every 200
      // frames, ns_core.c:262-270): its row is written back only then (wave-uniform branch)
      if (quant_new) STORE3(V_QUANT, quant)

      NS_STAMP(5)
      // ---- startup noise model (ns_core.c:1091-1100, 1109-1162)
      float whiteNoiseLevel = SC_F(S_WHITE);
      float pinkNoiseNumerator = SC_F(S_PINKNUM);
      float pinkNoiseExp = SC_F(S_PINKEXP);
      float fd5, fd6;
      {
        static_assert(S_FD6 == S_FD5 + 1, "read as a pair");
        float t2[2];
        srow.template ld<S_FD5, 2>(sv, t2);
        fd5 = t2[0]; fd6 = t2[1];
      }
      const bool startup = blockInd < NS_END_STARTUP_SHORT;
      if (startup) {
        const int binA_c = ns_cold(binA);
        const NsTables* Tc = ns_cold(T);
        float lm3[NS3], lilm[NS3];
#pragma unroll
        for (int k = 0; k < NS3; ++k) {
          const int bin = k < 2 ? binA_c + 32 * k : 128;
          const float li = Tc->logi[bin];
          lm3[k] = bin >= NS_START_BAND ? lmagn[k] : 0.f;
          lilm[k] = bin >= NS_START_BAND ? li * lmagn[k] : 0.f;
        }
        const float sum_log_magn = SUM3(lm3);
        const float sum_log_i_log_magn = SUM3(lilm);
        const NsPinkFit fit = ns_pink_fit<kBins>(Tc, whiteNoiseLevel, pinkNoiseNumerator, pinkNoiseExp, sumMagn,
                                                 SC_F(S_OVERDRIVE), sum_log_magn, sum_log_i_log_magn, blockInd);
        whiteNoiseLevel = fit.whiteNoiseLevel;
        pinkNoiseNumerator = fit.pinkNoiseNumerator;
        pinkNoiseExp = fit.pinkNoiseExp;
        float parametric_num = 0.f, parametric_exp = 0.f;
        if (pinkNoiseExp > 0.f) {
          parametric_num = (float)exp((double)(pinkNoiseNumerator / (float)(blockInd + 1)));
          parametric_num *= (float)(blockInd + 1);
          parametric_exp = pinkNoiseExp / (float)(blockInd + 1);
        }
        float pn[NS3];
#pragma unroll
        for (int k = 0; k < NS3; ++k) {
          const int bin = k < 2 ? binA_c + 32 * k : 128;
          if (pinkNoiseExp == 0.f) {
            pn[k] = whiteNoiseLevel;
          } else {
            const float use_band = (float)(bin < NS_START_BAND ? NS_START_BAND : bin);
            pn[k] = (float)((double)parametric_num / pow((double)use_band, (double)parametric_exp));
          }
          noise[k] *= (blockInd);
          const float t2 = pn[k] * (NS_END_STARTUP_SHORT - blockInd);
          noise[k] += (t2 / (float)(blockInd + 1));
          noise[k] /= NS_END_STARTUP_SHORT;
        }
        if constexpr (FLOW) {  // (a cold row: in memory, the lane's offset from the opaque copy)
          sa.st2(kOffVec + V_PARAMNOISE * kVecStride, 2 * ns_cold(lane), pn[0], pn[1]);
          SC_SET_F(S_TAIL0 + V_PARAMNOISE, pn[2]);
        } else {
          STORE3(V_PARAMNOISE, pn)
        }
      }
      fd5 = ns_startup_fd5(fd5, signalEnergy, blockInd);

      NS_STAMP(6)
      // ---- ComputeSnr (ns_core.c:566-588)
      {
        const f32x2 eps = {0.0001f, 0.0001f};
        const f32x2 ns2 = {noise[0], noise[1]}, mg2 = {magn[0], magn[1]};
        f32x2 stsa2;
        if (CARRY && carry_ok) {
          stsa2 = carry_stsa;
        } else {
          if constexpr (CARRY) { LOADV(magnPrevA, V_MAGNPREV_A) LOADV(smooth, V_SMOOTH) }
          const f32x2 q1 = fdiv2(f32x2{magnPrevA[0], magnPrevA[1]}, f32x2{noisePrev[0], noisePrev[1]} + eps);
          stsa2 = f32x2{q1[0] * smooth[0], q1[1] * smooth[1]};
        }
        const f32x2 d2 = ns2 + eps;
        f32x2 r2;
        if (RCPQ && STEADY && rcpq_ok) {
          r2 = rcpq;
        } else {
          r2 = fdiv2_rcp(d2);
          if constexpr (RCPQ && STEADY) asm volatile("; the quantile's reciprocal" : "+v"(r2));
        }
        if constexpr (RCPQ) {
          if constexpr (STEADY) rcpq = r2;
          rcpq_ok = STEADY;  // (a generic step may publish a quantile or blend the start-up model into the estimate)
        }
        const f32x2 q2 = fdiv2_quot(mg2, d2, r2);  // used where magn > noise
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float previousEstimateStsa = stsa2[k];
          prevStsa[k] = previousEstimateStsa;
          snrLocPost[k] = 0.f;
          if (magn[k] > noise[k]) snrLocPost[k] = q2[k] - 1.f;
          snrLocPrior[k] = NS_DD_PR_SNR * previousEstimateStsa + (1.f - NS_DD_PR_SNR) * snrLocPost[k];
        }
        if constexpr (!STEADY) snr_tail(noise[2]);
      }

      NS_STAMP(7)
      // ---- ComputeSpectralFlatness (ns_core.c:523-556)
      // (featureData[0], [3] and [4] are read from the scalar row in front of their first use)
      static_assert(S_PMP5 == S_PMP4 + 1 && S_PMP1 == S_PMP0 + 1 && S_PMP2 == S_PMP0 + 2 && S_PMP3 == S_PMP0 + 3,
                    "scalars read as groups");
      PriorModel pm;
      float fd4 = SC_F(S_FD4);
      [[maybe_unused]] NsDiffArgs diffa;
      [[maybe_unused]] float diff_varMagn;
      // (its exponential is evaluated beside bin 128's of exp(-logLrt), each on a lane of one call, once logLrt is
      // updated: the feature is finished there, in front of its first readers, the histogram and the tanh)
      const NsFlatArgs flat = ns_flatness_args<kBins>(flatNum, sumMagn, lane_bcast(magn[0], 0));
      // ---- ComputeSpectralDifference (ns_core.c:595-634)
      {
        float avgMagn = sumMagn;
        {  // two independent wave-uniform quotients by the bin count: DIV129's three operations, packed
          const f32x2 q = DIV129_2((f32x2{avgPauseMean, avgMagn}));
          avgPauseMean = q.x;
          avgMagn = q.y;
        }
        float cv[NS3], vp[NS3], vm[NS3];
#pragma unroll
        for (int k = 0; k < NS3; ++k) {
          const float dm = magn[k] - avgMagn, dp = avgPause[k] - avgPauseMean;
          cv[k] = dm * dp;
          vp[k] = dp * dp;
          vm[k] = dm * dm;
        }
        float covMagnPause = cv[0] + cv[1], varPause = vp[0] + vp[1], varMagn = vm[0] + vm[1];
        wave_sums_bcast(covMagnPause, varPause, varMagn);
        covMagnPause += cv[2];
        varPause += vp[2];
        varMagn += vm[2];
        {
          const f32x2 q = DIV129_2((f32x2{covMagnPause, varPause}));
          covMagnPause = q.x;
          varPause = q.y;
        }
        varMagn = DIV129(varMagn);
        fd6 += signalEnergy;
        // (its two quotients are divided in phase 8, each beside another wave-uniform quotient that is independent of
        // it: the first with bin 128's of the likelihood ratio, the second with the flatness feature's)
        diffa = ns_spectral_diff_args(covMagnPause, varPause, fd5);
        diff_varMagn = varMagn;
      }

      NS_STAMP(8)
      // ---- SpeechNoiseProb (ns_core.c:642-749): the likelihood-ratio update
      {
        float t1[NS3], lt1[NS3];
        LOADT(logLrt, V_LOGLRT)
#pragma unroll
        for (int k = 0; k < NS3; ++k) t1[k] = 1.f + 2.f * snrLocPrior[k];
        if constexpr (STEADY) {
          const float t1p[2] = {t1[0], t1[1]};
          float lt1p[2];
          // (the per-lane form: this is the step's widest point, and the wave-level form of these two chains costs the
          // hand-off product kernels three spilled vector registers, profiles/README.md)
          log_f32_via_tab_n<2, true>(t1p, lt1p, logts);
          lt1[0] = lt1p[0]; lt1[1] = lt1p[1];
          lt1[2] = lt1_tail;
        } else {
          log_f32_via_tab_n_wave<NS3>(t1, lt1, logts);
        }
        float tn[NS3], td3[NS3], t2v[NS3];
#pragma unroll
        for (int k = 0; k < NS3; ++k) {
          tn[k] = 2.f * snrLocPrior[k];
          td3[k] = t1[k] + 0.0001f;
        }
        {
          const f32x2 a = fdiv2(f32x2{tn[0], tn[1]}, f32x2{td3[0], td3[1]});
          const f32x2 b = fdiv2(f32x2{tn[2], diffa.n1}, f32x2{td3[2], diffa.d1});
          t2v[0] = a.x; t2v[1] = a.y; t2v[2] = b.x;
          diffa.n1 = diff_varMagn - b.y;  // avgDiffNormMagn's numerator (ns_core.c:630)
        }
#pragma unroll
        for (int k = 0; k < NS3; ++k) {
          const float t2 = t2v[k];
          const float besselTmp = (snrLocPost[k] + 1.f) * t2;
          logLrt[k] += NS_LRT_TAVG * (besselTmp - lt1[k] - logLrt[k]);
        }
      }
      float logLrtTimeAvgKsum = SUM3(logLrt);
      logLrtTimeAvgKsum = DIV129(logLrtTimeAvgKsum);
      // exp(-logLrt) of the lane's two bins, and two independent wave-uniform exponentials in the third slot of the
      // same call: the flatness feature's on lane 0, bin 128's on every other lane (read back from lane 1)
      // (the scalars of the prior-model map, phase 9, are requested in front of the exponentials, whose table reads wait
      // anyway: featureData[0] and [3] -- the previous frame's average LRT, for the histogram -- and the model's first four)
      float ev[NS3], fd0 = SC_F(S_FD0), fd3 = SC_F(S_FD3), pmp2;
      {
        float t4[4];
        srow.template ld<S_PMP0, 4>(sv, t4);
        pm.p0 = t4[0]; pm.p1 = t4[1]; pmp2 = t4[2]; pm.p3 = t4[3];
        pm.p4 = pm.p5 = pm.p6 = 0.f;  // (the three weights: read in front of the tanh, unless the window closes here and sets them)
      }
      {
        float nl[NS3];
#pragma unroll
        for (int k = 0; k < NS3; ++k) nl[k] = -logLrt[k];
        nl[2] = lane == 0 ? flat.arg : nl[2];
        exp_f32_via_f64_n_wave<NS3>(nl, ev, exp2s);
        {
          const f32x2 qq = fdiv2(f32x2{lane_bcast(ev[2], 0), diffa.n1}, f32x2{flat.den, diffa.d2});
          fd0 = ns_flatness_update_q(fd0, qq.x);  // ns_core.c:551-555
          fd4 = ns_spectral_diff_q(fd4, qq.y);    // ns_core.c:631-634
        }
        ev[2] = lane_bcast(ev[2], 1);
      }

      NS_STAMP(9)
      // ---- histograms / prior model (FeatureUpdate, ns_core.c:766-790): the new flatness and difference features, the
      // previous frame's average LRT
      int mup0 = updateParsFlag, mup3 = ss.mup3;
      const int mup1 = SC_I(S_MUP1);
      bool window_closed = false;
      if constexpr (DEFER && !STEADY) hist_flush();  // a generic step counts what is pending, then does what it did
      if constexpr (STEADY && DEFER) {
        // the steady body adds in every step (updateParsFlag >= 1, mup3 > 2) and closes no window: the three features
        // as they stand here go into the step's slot, from lane 0; hist_flush() counts them
        const unsigned rel = LIST ? flow_j : flow_j - blockIdx.y * fa.walk;  // the step of the walk
        // (past the walk's first kPendSteps steps a slot may be taken -- which ones depends on the zero-energy and
        // generic steps behind -- so every record counts what is pending first; the product's walks are 4 and 8 steps)
        if (rel >= (unsigned)kPendSteps) hist_flush();
        mup3--;
        if (lane == 0) {
          lds_f32* const slot = pend + 3 * (rel & (kPendSteps - 1));
          slot[0] = fd3; slot[1] = fd0; slot[2] = fd4;
        }
      } else if (updateParsFlag >= 1) {
        mup3--;
        if (mup3 > 0) {
          // FeatureParameterExtraction(self, 0), ns_core.c:309-334: lanes 0..2 take one histogram each
          // (LRT, spectral flatness, spectral difference); one writer per bin and stream, so a
          // no-return atomic add is the increment without the load -> add -> store round trip
          const int lane_c = ns_cold(lane);
          const float fv = lane_c == 0 ? fd3 : (lane_c == 1 ? fd0 : fd4);
          const float bw = lane_c == 1 ? 0.05f : 0.1f, rbw = lane_c == 1 ? 1.0f / 0.05f : 1.0f / 0.1f;
          const float lim = lane_c == 1 ? kHist * 0.05f : kHist * 0.1f;
          if (lane_c < 3 && (fv < lim) && (fv >= 0.0f))
            atomicAdd(&hist[lane_c * kHistStride + (int)div_by_uniform(fv, bw, rbw)], 1);  // agent scope (sc1)
        }
        if (mup3 == 0) {
          // hand-off build: the no-return increments of the walk's earlier steps are complete before the window is
          // read, and its clearing stores before the next step's increment
          if constexpr (FLOW) handoff_drain();
          pm = close_histogram_window<FLOW>(hist, lane, mup1, mup0 >= 1, pm);
          if constexpr (FLOW) handoff_drain();
          window_closed = true;
          const NsWindowOpen wo = ns_window_reopen(updateParsFlag, mup1, fd5, fd6);
          mup0 = wo.mup0;
          mup3 = wo.mup3;
          fd5 = wo.fd5;
          fd6 = wo.fd6;
        }
      }
      fd3 = logLrtTimeAvgKsum;
      {
        if (!window_closed) {
          float t2[2];
          srow.template ld<S_PMP4, 2>(sv, t2);
          pm.p4 = t2[0]; pm.p5 = t2[1];
          pm.p6 = SC_F(S_PMP6);
        }
        priorSpeechProb = SC_F(S_PRIORSPEECHPROB);
        const float widthPrior0 = NS_WIDTH_PR_MAP, widthPrior1 = 2.f * NS_WIDTH_PR_MAP,
                    widthPrior2 = 2.f * NS_WIDTH_PR_MAP;
        const int sgnMap = (int)pmp2;
        float widthPrior = widthPrior0;
        if (logLrtTimeAvgKsum < pm.p0) widthPrior = widthPrior1;
        const float arg0 = widthPrior * (logLrtTimeAvgKsum - pm.p0);
        widthPrior = widthPrior0;
        if (sgnMap == 1 && (fd0 > pm.p1)) widthPrior = widthPrior1;
        if (sgnMap == -1 && (fd0 < pm.p1)) widthPrior = widthPrior1;
        const float arg1 = (float)sgnMap * widthPrior * (pm.p1 - fd0);
        widthPrior = widthPrior0;
        if (fd4 < pm.p3) widthPrior = widthPrior2;
        const float arg2 = widthPrior * (fd4 - pm.p3);
        // the three tanh() of :696-725 evaluated on lanes 0..2 of one call
        const float arg = lane == 0 ? arg0 : (lane == 1 ? arg1 : arg2);
        const float th = tanh_f32_via_f64_wave(arg, exp2s);
        priorSpeechProb = ns_prior_update(priorSpeechProb, pm, ns_prior_indicator(lane_bcast(th, 0)),
                                          ns_prior_indicator(lane_bcast(th, 1)), ns_prior_indicator(lane_bcast(th, 2)));
      }
      float probSpeech[NS3];
      {
        // one free operand, priorSpeechProb in [0.01, 1] behind its clamps: the one-correction chain is fdiv's quotient
        const float gainPrior = fdiv_1c(1.f - priorSpeechProb, priorSpeechProb + 0.0001f);
        {
          float pd[NS3];
#pragma unroll
          for (int k = 0; k < NS3; ++k) {
            float invLrt = ev[k];
            invLrt = (float)gainPrior * invLrt;
            pd[k] = 1.f + invLrt;
          }
          // 1 / pd: the numerator is 1, the reciprocal chain is the quotient's (frcp == fdiv(1.f, .) on every float)
          const f32x2 ps2 = frcp2(f32x2{pd[0], pd[1]});
          probSpeech[0] = ps2.x; probSpeech[1] = ps2.y;
          probSpeech[2] = frcp(pd[2]);
        }
      }

      NS_STAMP(10)
      // ---- UpdateNoiseEstimate (ns_core.c:800-846): the time constant carried into bin i is the one
      // bin i-1 selected.  For q > 0 bin i-1 is the same slot of lane L - 2; for q == 0 it is bin
      // 15 + 16 (t - 1) + 64 g (t > 0) or bin 63 (bin 64), i.e. a slot of lane 30 / 31 (+ 32 g):
      //   slot 0 (t = h):     h = 1: lane 30 + 32 g slot 0;   h = 0, g = 1: lane 31 slot 1;   bin 0: none
      //   slot 1 (t = h + 2): h = 0: lane 31 + 32 g slot 0;   h = 1: lane 30 + 32 g slot 1
      {
        const int srcA = q > 0 ? lane - 2 : (h ? 30 + 32 * g : 31);
        const int srcB = q > 0 ? lane - 2 : (h ? 30 + 32 * g : 31 + 32 * g);
        const bool a_from1 = q == 0 && h == 0;  // slot 0 takes the source lane's slot 1
        const bool b_from1 = q > 0 || h == 1;   // slot 1 takes the source lane's slot 1
        const float a0 = __shfl(probSpeech[0], srcA, 64), a1 = __shfl(probSpeech[1], srcA, 64);
        const float b0 = __shfl(probSpeech[0], srcB, 64), b1 = __shfl(probSpeech[1], srcB, 64);
        float prevProb[NS3];
        prevProb[0] = a_from1 ? a1 : a0;
        prevProb[1] = b_from1 ? b1 : b0;
        prevProb[2] = lane_bcast(probSpeech[1], 63);  // bin 128 <- bin 127 (q = 15, g = 1, t = 3)
        // ns_core.c:813-845.  The update with a time constant g is u(g) = g noisePrev + (1 - g) x, x = (1 -
        // ps) magn + ps noisePrev; the reference computes u(gammaOld) and, when gammaNew differs, keeps the
        // smaller of u(gammaOld) and u(gammaNew).  With both constants' updates at hand that is: the old
        // bin's choice, the new bin's choice, their minimum (equal choices give the same value twice).
        {
          const F3 np(noisePrev), mg(magn), ps(probSpeech), ap(avgPause);
          const F3 x = (1.f - ps) * mg + ps * np;
          const F3 uS = NS_SPEECH_UPDATE * np + (1.f - NS_SPEECH_UPDATE) * x;
          const F3 uN = NS_NOISE_UPDATE * np + (1.f - NS_NOISE_UPDATE) * x;
          B3 oldSpeech = gt3(F3(prevProb), F3(NS_PROB_RANGE));
          oldSpeech.v[0] = oldSpeech.v[0] && lane != 0;  // bin 0 has no predecessor: gamma = NOISE_UPDATE
          const F3 uOld = sel3(oldSpeech, uS, uN);
          const F3 uNew = sel3(gt3(ps, F3(NS_PROB_RANGE)), uS, uN);
          min3(uOld, uNew).store(noise);
          sel3(lt3(ps, F3(NS_PROB_RANGE)), ap + NS_GAMMA_PAUSE * (mg - ap), ap).store(avgPause);
        }
      }
      STORE3_HOT(V_LOGLRT, logLrt) STORE3_HOT(V_AVGPAUSE, avgPause)
      STORE3_HOT(V_MAGNPREV_A, magn)  // ns_core.c:1180 (== magnPrevProcess while paired)

      NS_STAMP(11)
      // ---- Process: decision-directed Wiener gain (ns_core.c:985-1007, 1276-1307)
      float initMagn[NS3], pnoise[NS3];
      if (startup) {  // ns_core.c:1268-1272
        if constexpr (FLOW) {
          // the two cold rows stay in memory and are written and read back inside a walk: the wave's stores to them
          // (this step's V_PARAMNOISE, the previous step's V_INITMAGN) are complete before it reads
          handoff_drain();
          const int lane2_c = 2 * ns_cold(lane);
          const float2 im_ = sa.ld2(kOffVec + V_INITMAGN * kVecStride, lane2_c);
          const float2 pn_ = sa.ld2(kOffVec + V_PARAMNOISE * kVecStride, lane2_c);
          initMagn[0] = im_.x; initMagn[1] = im_.y;
          pnoise[0] = pn_.x; pnoise[1] = pn_.y;
          LOADT(initMagn, V_INITMAGN) LOADT(pnoise, V_PARAMNOISE)
#pragma unroll
          for (int k = 0; k < NS3; ++k) initMagn[k] += magn[k];
          sa.st2(kOffVec + V_INITMAGN * kVecStride, lane2_c, initMagn[0], initMagn[1]);
          SC_SET_F(S_TAIL0 + V_INITMAGN, initMagn[2]);
        } else {
          LOAD3(initMagn, V_INITMAGN)
          LOAD3(pnoise, V_PARAMNOISE)
#pragma unroll
          for (int k = 0; k < NS3; ++k) initMagn[k] += magn[k];
          STORE3(V_INITMAGN, initMagn)
        }
      }
      float overdrive, denoiseBound;
      {
        static_assert(S_DENOISEBOUND == S_OVERDRIVE + 1, "scalars read as a pair");
        float t2[2];
        srow.template ld<S_OVERDRIVE, 2>(sv, t2);
        overdrive = t2[0]; denoiseBound = t2[1];
      }
      float gainv[NS3];
      float gq1[NS3], gq2[NS3], snrP[NS3];
      {
        float gd1[NS3], gd2[NS3];
#pragma unroll
        for (int k = 0; k < NS3; ++k) gd1[k] = noise[k] + 0.0001f;
        fdiv3(magn, gd1, gq1);  // used where magn > noise
#pragma unroll
        for (int k = 0; k < NS3; ++k) {
          float currentEstimateStsa = 0.f;
          if (magn[k] > noise[k]) currentEstimateStsa = gq1[k] - 1.f;
          snrP[k] = NS_DD_PR_SNR * prevStsa[k] + (1.f - NS_DD_PR_SNR) * currentEstimateStsa;
          gd2[k] = overdrive + snrP[k];
        }
        fdiv3(snrP, gd2, gq2);
      }
#pragma unroll
      for (int k = 0; k < NS3; ++k) {
        float gg = fmin_raw(fmax_raw(gq2[k], denoiseBound), 1.f);  // ns_core.c:1001-1006
        if (startup) {
          float tmp = (initMagn[k] - overdrive * pnoise[k]);
          tmp /= (initMagn[k] + 0.0001f);
          if (tmp < denoiseBound) tmp = denoiseBound;
          if (tmp > 1.f) tmp = 1.f;
          gg *= (blockInd);
          tmp *= (NS_END_STARTUP_SHORT - blockInd);
          gg += tmp;
          gg /= (NS_END_STARTUP_SHORT);
        }
        gainv[k] = gg;
        re[k] *= gg;
        im[k] *= gg;
      }
      if constexpr (CARRY) {  // the next step's previous-frame estimate, from the values the three rows are stored from
        carry_stsa = f32x2{gq1[0], gq1[1]} * f32x2{gainv[0], gainv[1]};
        carry_stsa_tail = gq1[2] * gainv[2];
        carry_ok = true;
      }
      STORE3_HOT(V_SMOOTH, gainv)      // ns_core.c:1304
      STORE3_HOT(V_NOISEPREV, noise)   // ns_core.c:1310
      // ---- commit the float scalars: every one is final here.  The hand-off build stores them to the image now, on
      // lane 0 alone, with the bin-128 members of the five rows above; the plain build merges them into `sv` at the
      // step's end, where it always did
      auto commit_floats = [&]() __attribute__((always_inline)) {
        if constexpr (ROW_IMG) {
          SC_SET_F(S_TAIL0 + V_LOGLRT, logLrt[2]);
          SC_SET_F(S_TAIL0 + V_AVGPAUSE, avgPause[2]);
          SC_SET_F(S_TAIL0 + V_MAGNPREV_A, magn[2]);
          SC_SET_F(S_TAIL0 + V_SMOOTH, gainv[2]);
          SC_SET_F(S_TAIL0 + V_NOISEPREV, noise[2]);
        }
        SC_SET_F(S_SIGNALENERGY, signalEnergy);
        SC_SET_F(S_SUMMAGN, sumMagn);
        if (startup) {
          SC_SET_F(S_WHITE, whiteNoiseLevel);
          SC_SET_F(S_PINKNUM, pinkNoiseNumerator);
          SC_SET_F(S_PINKEXP, pinkNoiseExp);
        }
        if (window_closed) {
          SC_SET_F(S_PMP0, pm.p0);
          SC_SET_F(S_PMP1, pm.p1);
          SC_SET_F(S_PMP3, pm.p3);
          SC_SET_F(S_PMP4, pm.p4);
          SC_SET_F(S_PMP5, pm.p5);
          SC_SET_F(S_PMP6, pm.p6);
        }
        SC_SET_F(S_FD0, fd0);
        SC_SET_F(S_FD3, fd3);
        SC_SET_F(S_FD4, fd4);
        SC_SET_F(S_FD5, fd5);
        SC_SET_F(S_FD6, fd6);
        SC_SET_F(S_PRIORSPEECHPROB, priorSpeechProb);
      };
      if constexpr (ROW_IMG) {
        if (lane == 0) commit_floats();
      }

      NS_STAMP(12)
      NS_NEXT_FRAME()
      // ---- IFFT (ns_core.c:923-944)
      er = f32x2{re[0], re[1]};
      ei = f32x2{im[0], im[1]};
      if (lane == 0) ei.x = re[2];  // Ooura packing: a[1] = R128
      real_split1(tile, spls, lane, er, ei, true);
      lds_sync1();
      {
        const int base = 64 * g + q + 16 * h;
        float* tf = reinterpret_cast<float*>(tile);
        tf[2 * base] = er.x;
        tf[2 * base + 1] = ei.x;
        tf[2 * base + 64] = er.y;
        tf[2 * base + 65] = ei.y;
      }
      lds_sync1();
      f32x2 tr, ti;  // samples 2E (tr) and 2E + 1 (ti) of elements E = binA (slot 0) and binA + 32 (slot 1)
      {
        f32x2 ea, eb;
        cft128_passes1(tile, tws, fl, lane, ea, eb);
        radix2_tail1(ea, eb, gmask, true, tr, ti);
      }
      const float td0 = tr.x * (2.f / kAnal), td1 = ti.x * (2.f / kAnal);
      const float td2 = tr.y * (2.f / kAnal), td3s = ti.y * (2.f / kAnal);

      NS_STAMP(13)
      // ---- energy-based gain compensation (ns_core.c:1315-1342)
      float factor = 1.f;
      if (gainmap == 1 && blockInd > NS_END_STARTUP_LONG) {
        float e2 = td0 * td0;
        e2 += td1 * td1;
        e2 += td2 * td2;
        e2 += td3s * td3s;
        factor = ns_gain_factor<true>(wave_sum_bcast(e2), energy1, denoiseBound, priorSpeechProb);
      }

      // ---- synthesis window, overlap-add, emit 160, carry 96 (ns_core.c:1344-1359)
      {
        float* y = IO16 ? reinterpret_cast<float*>(reinterpret_cast<short*>(outj) + (size_t)stream * kBlockL)
                        : outj + (size_t)stream * kBlockL;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int nA = 2 * ns_cold(binA), nB = nA + 64;  // sample index of td0 / td2
        const float2 wA = *reinterpret_cast<const float2*>(wins + nA);
        const float2 wB = *reinterpret_cast<const float2*>(wins + nB);
        const float cA0 = g == 0 ? carryA.x : 0.f, cA1 = g == 0 ? carryA.y : 0.f;
        const float cB0 = (g == 0 && h == 0) ? carryB.x : 0.f, cB1 = (g == 0 && h == 0) ? carryB.y : 0.f;
        const float oA0 = cA0 + factor * (wA.x * td0), oA1 = cA1 + factor * (wA.y * td1);
        const float oB0 = cB0 + factor * (wB.x * td2), oB1 = cB1 + factor * (wB.y * td3s);
        // Saturation of the emitted samples (ns_core.c:1352-1356) behind ONE wave-level test: a value with
        // |x| <= 32767 is what sat16p returns for it, so where no lane holds another the values are stored as they are;
        // otherwise -- x > 32767, x < -32767, a NaN, on any lane, the synthesis tail's included -- the same stores with
        // sat16p, out of line.  The tail in LDS is stored unsaturated either way.
        auto emit = [&](auto sat_c) __attribute__((always_inline)) {
          constexpr bool SAT = decltype(sat_c)::value;
          if (nA >= 160) {
            sa.st2(kOffSynt, nA - 160, oA0, oA1);
          } else {
            store2p<IO16>(y, nA, SAT ? sat16p(oA0) : oA0, SAT ? sat16p(oA1) : oA1);
          }
          if (nB >= 160) {
            sa.st2(kOffSynt, nB - 160, oB0, oB1);
          } else {
            store2p<IO16>(y, nB, SAT ? sat16p(oB0) : oB0, SAT ? sat16p(oB1) : oB1);
          }
        };
        // (one compare's lane mask per value, OR-ed with scalar instructions)
        const unsigned long long may_clip =
            (__builtin_amdgcn_ballot_w64(sat16p_may_clip(oA0)) | __builtin_amdgcn_ballot_w64(sat16p_may_clip(oA1))) |
            (__builtin_amdgcn_ballot_w64(sat16p_may_clip(oB0)) | __builtin_amdgcn_ballot_w64(sat16p_may_clip(oB1)));
        if (ASP_NS_RARE(may_clip != 0)) emit(std::true_type{});
        else emit(std::false_type{});
      }

      NS_STAMP(14)
      // ---- commit scalars
      if constexpr (STEADY) {
        sv = addlanes_bits<(1ull << S_BLOCKIND) | (7ull << S_COUNTER0), 1ull << S_MUP3>(sv);
      } else {
        SC_SET_I(S_UPDATES, updates);
        SC_SET_I(S_COUNTER0, counter[0]);
        SC_SET_I(S_COUNTER1, counter[1]);
        SC_SET_I(S_COUNTER2, counter[2]);
        SC_SET_I(S_MUP0, mup0);
        SC_SET_I(S_MUP3, mup3);
        SC_SET_I(S_BLOCKIND, blockInd);
      }
      if constexpr (!ROW_IMG) commit_floats();
    };  // step_rest
    if (__builtin_expect(step_steady, 1)) step_rest(std::true_type{});
    else step_rest(std::false_type{});
    if constexpr (!FLOW) sa.st1(kOffScalars, lane, sv);  // (hand-off build: with the image, at the walk's end)
    NS_STAMP(15)
    NS_STREAM_DONE(0)
  }
#undef NS_STREAM_DONE
#undef NS_NEXT_FRAME
#undef NS_STAMP
#undef NS_BUDGET_ASIDE
#undef NS_BUDGET_BACK
#undef SC_I
#undef SC_F
#undef SC_SET_I
#undef SC_SET_F
#undef LOAD3
#undef LOADV
#undef LOADT
#undef STORE3
#undef STORE3_HOT
#undef SUM3
}

// the product kernels: the four DIAG = false instantiations
template <bool IO16, bool FLOW>
__global__ __launch_bounds__(256, 4) void ns_frame1_kernel(float* __restrict__ state,
                                                           int32_t* __restrict__ hist_all,
                                                           const NsTables* __restrict__ T,
                                                           const float* __restrict__ in,
                                                           float* __restrict__ out,
                                                           int num_streams, int steady_on, NsFlowArgs fa) {
  ns_frame1_run<IO16, FLOW, false>(state, hist_all, T, in, out, num_streams, steady_on, fa, NsDiagArgs{nullptr, 0});
}

// the list kernels (NsListArgs): the hand-off body's product step on the listed streams, float and int16 frames
template <bool IO16>
__global__ __launch_bounds__(256, 4) void ns_list1_kernel(float* __restrict__ state, int32_t* __restrict__ hist_all,
                                                          const NsTables* __restrict__ T,
                                                          const float* __restrict__ in, float* __restrict__ out,
                                                          int steady_on, NsFlowArgs fa, NsListArgs la) {
  ns_frame1_run<IO16, true, false, true>(state, hist_all, T, in, out, la.n, steady_on, fa, NsDiagArgs{nullptr, 0}, la);
}

// the diagnostic kernels (stamps, timeline, step counts): float frames only, which is what their entry points use
template <bool FLOW>
__global__ __launch_bounds__(256, 4) void ns_frame1_diag_kernel(float* __restrict__ state,
                                                                int32_t* __restrict__ hist_all,
                                                                const NsTables* __restrict__ T,
                                                                const float* __restrict__ in,
                                                                float* __restrict__ out,
                                                                int num_streams, int steady_on, NsFlowArgs fa,
                                                                NsDiagArgs dg) {
  ns_frame1_run<false, FLOW, true>(state, hist_all, T, in, out, num_streams, steady_on, fa, dg);
}

// Test seam: the frame step's tanh (tanh_f32_via_f64_wave, which only this file uses) against (float)tanh((double)x) on
// every float whose bit pattern is in [start, start + count); the protocol of ns_kernels.hip's debug_compare_kernel.
__global__ void debug_tanh_wave_kernel(unsigned start, unsigned count, unsigned* n_bad, unsigned* bad_bits,
                                       const NsTables* __restrict__ T) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float x = __uint_as_float(start + i);
  const float a = tanh_f32_via_f64_wave(x, T->exp2_64), b = (float)tanh((double)x);
  const bool same = (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b);
  if (!same) {
    const unsigned k = atomicAdd(n_bad, 1u);
    if (k < 64) bad_bits[k] = start + i;
  }
}

// Test seam: the frame step's wave-level guards on every float whose bit pattern is in [start, start + count), 64
// consecutive patterns to a wave -- the emitted sample (stored as it is unless sat16p_may_clip holds on some lane of the
// wave, through sat16p otherwise) against sat16p, and fsqrt_wave against sqrtf.
__global__ void debug_guards_wave_kernel(unsigned start, unsigned count, unsigned* n_bad, unsigned* bad_bits) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float x = __uint_as_float(start + i);
  float emitted = x;
  if (__builtin_amdgcn_ballot_w64(sat16p_may_clip(x)) != 0) emitted = sat16p(x);
  const float a = fsqrt_wave(x), b = sqrtf(x);
  const bool same = __float_as_uint(emitted) == __float_as_uint(sat16p(x)) &&
                    ((__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b));
  if (!same) {
    const unsigned k = atomicAdd(n_bad, 1u);
    if (k < 64) bad_bits[k] = start + i;
  }
}

// Test seam: the steady step's wave-level libm fallbacks and its reciprocal chain, on every 32-bit pattern in [start,
// start + count), 64 consecutive patterns to a wave.  `what`:
//   0  the pattern as the low word of an fp64 value: the two-instruction rounding test against the negation of
//      f64_rounds_safely_to_f32's
//   1  frcp and both halves of frcp2 against fdiv(1.f, x), bit for bit (NaN payloads included)
//   2 / 3  log_f32_via_tab_n_wave against log_f32_via_tab: the pattern alone on one lane of the wave with a benign
//      argument (1.5f) on the 63 others, for each lane in turn -- the others' results are checked too, so a fallback
//      that one lane provokes must leave them what they had -- / 64 consecutive patterns on the wave's lanes
//   4 / 5  exp_f32_via_f64_n_wave against exp_f32_via_f64 in the same two arrangements (benign argument: 0.5f)
// Both sides of every wave-level branch are met: a wave of positive normal (log) or in-range (exp) patterns is flagged
// in about 2 of 10 000 cases, a wave of negative or NaN patterns always.
__global__ void debug_fallbacks_wave_kernel(int what, unsigned start, unsigned count, unsigned* n_bad,
                                            unsigned* bad_bits, const NsTables* __restrict__ T) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < count;  // (no early return: the one-lane arrangements loop over the wave's lanes)
  const unsigned bits = start + (live ? i : 0u);
  const float x = __uint_as_float(bits);
  const double2* lt = reinterpret_cast<const double2*>(T->logtab);
  auto eq = [](float a, float b) { return (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b); };
  bool same = true;
  if (what == 0) {
    const unsigned lo = bits & 0x1fffffffu;
    same = f64_lo_rounds_unsafely(bits) == !((lo - 0x0ffffe00u) > 0x400u);
  } else if (what == 1) {
    const float want = fdiv(1.f, x);
    const f32x2 a = frcp2(f32x2{x, 1.5f}), b = frcp2(f32x2{3.f, x});
    same = __float_as_uint(frcp(x)) == __float_as_uint(want) && __float_as_uint(a.x) == __float_as_uint(want) &&
           __float_as_uint(b.y) == __float_as_uint(want) && __float_as_uint(a.y) == __float_as_uint(fdiv(1.f, 1.5f)) &&
           __float_as_uint(b.x) == __float_as_uint(fdiv(1.f, 3.f));
  } else if (what == 2 || what == 4) {
    const bool is_log = what == 2;
    const float benign = is_log ? 1.5f : 0.5f;
    const float want = is_log ? log_f32_via_tab(x, lt) : exp_f32_via_f64(x, T->exp2_64);
    const float want_benign = is_log ? log_f32_via_tab(benign, lt) : exp_f32_via_f64(benign, T->exp2_64);
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < 64; ++j) {
      const float in[1] = {lane == j ? x : benign};
      float o[1];
      if (is_log) log_f32_via_tab_n_wave<1>(in, o, lt);
      else exp_f32_via_f64_n_wave<1>(in, o, T->exp2_64);
      same = same && eq(o[0], lane == j ? want : want_benign);
    }
  } else if (what == 3) {
    const float in[1] = {x};
    float o[1];
    log_f32_via_tab_n_wave<1>(in, o, lt);
    same = eq(o[0], log_f32_via_tab(x, lt));
  } else {
    const float in[1] = {x};
    float o[1];
    exp_f32_via_f64_n_wave<1>(in, o, T->exp2_64);
    same = eq(o[0], exp_f32_via_f64(x, T->exp2_64));
  }
  if (live && !same) {
    const unsigned k = atomicAdd(n_bad, 1u);
    if (k < 64) bad_bits[k] = bits;
  }
}

// Test seam: the steady step's short division chains (ns_device.h: fdiv_c, fdiv_1c, div_by_uniform2; ns_step.h: fdiv40)
// and the logarithm's one-instruction argument reduction, each beside the form it replaces, on every 32-bit pattern in
// [start, start + count), 64 consecutive patterns to a wave; bits are compared, or NaN-ness on both sides.  `what`:
//   0  fdiv40 and both halves of fdiv40_2 against fdiv(FACTOR, d), d = max(pattern, 1) as the trackers form it (+inf and
//      NaNs included)
//   1  gainPrior: the pattern as priorSpeechProb through ns_prior_update's clamps, then fdiv_1c against fdiv of
//      (1 - p) / (p + 0.0001f)
//   2  the logarithm: the pattern as the argument's bits through log_reduced_bits_mad against the AND and subtract, and
//      log_f32_via_tab_n<1, true> against log_f32_via_tab
//   3  both halves of div_by_uniform2 against div_by_uniform, divisor 129 (the bin count) and its rounded reciprocal
//   4  fsqrt_wave (one correction of x r) against fsqrt (g and h refined first) on every pattern of a non-negative
//      float or a NaN -- tiny arguments, zero and +inf through both forms' own branches
// Candidates that do NOT ship (their counts are recorded, profiles/README.md; nothing in the step calls them):
//   5  the phase-8 quotient tn / ((1 + tn) + 0.0001f), tn = 2 * pattern (snrLocPrior), fdiv_1c against fdiv
//   6  fsqrt's chain with only h unrefined, for arguments in [2^-100, inf)
__global__ void debug_shortdiv_wave_kernel(int what, unsigned start, unsigned count, unsigned* n_bad,
                                           unsigned* bad_bits, const NsTables* __restrict__ T) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const unsigned bits = start + i;
  const float x = __uint_as_float(bits);
  auto eq = [](float a, float b) { return (__float_as_uint(a) == __float_as_uint(b)) || (a != a && b != b); };
  bool same = true;
  if (what == 0) {
    const float d = fmax_raw(x, 1.0f), fac = NS_FACTOR * 1.f;
    const float want = fdiv(fac, d);
    const f32x2 a = fdiv40_2(f32x2{d, 1.5f}), b = fdiv40_2(f32x2{3.f, d});
    same = eq(fdiv40(d), want) && eq(a.x, want) && eq(b.y, want) && eq(a.y, fdiv(fac, 1.5f)) && eq(b.x, fdiv(fac, 3.f));
  } else if (what == 1) {
    float p = x;
    if (p > 1.f) p = 1.f;
    if (p < 0.01f) p = 0.01f;
    same = eq(fdiv_1c(1.f - p, p + 0.0001f), fdiv(1.f - p, p + 0.0001f));
  } else if (what == 2) {
    const unsigned tmp = bits - kLogOff;
    same = log_reduced_bits_mad((int)tmp >> 23, bits) == bits - (tmp & 0xff800000u);
    const double2* lt = reinterpret_cast<const double2*>(T->logtab);
    const float in[1] = {x};
    float o[1];
    log_f32_via_tab_n<1, true>(in, o, lt);
    same = same && eq(o[0], log_f32_via_tab(x, lt));
  } else if (what == 3) {
    const float nb = (float)kBins, rnb = 1.0f / (float)kBins;
    const float want = div_by_uniform(x, nb, rnb);
    const f32x2 a = div_by_uniform2(f32x2{x, 1.5f}, nb, rnb), b = div_by_uniform2(f32x2{3.f, x}, nb, rnb);
    same = eq(a.x, want) && eq(b.y, want) && eq(a.y, div_by_uniform(1.5f, nb, rnb)) &&
           eq(b.x, div_by_uniform(3.f, nb, rnb));
  } else if (what == 4) {
    if ((bits >> 31) == 0u || x != x) same = eq(fsqrt_wave(x), fsqrt(x));
  } else if (what == 5) {
    const float tn = 2.f * x, t1 = 1.f + tn;
    same = eq(fdiv_1c(tn, t1 + 0.0001f), fdiv(tn, t1 + 0.0001f));
  } else {
    if (x >= 0x1p-100f && x < __builtin_inff()) {
      const float r = __builtin_amdgcn_rsqf(x);
      float g = x * r;
      const float h = 0.5f * r;
      const float e = __builtin_fmaf(-h, g, 0.5f);
      g = __builtin_fmaf(g, e, g);
      const float d = __builtin_fmaf(-g, g, x);
      same = eq(__builtin_fmaf(d, h, g), fsqrt(x));
    }
  }
  if (!same) {
    const unsigned k = atomicAdd(n_bad, 1u);
    if (k < 64) bad_bits[k] = bits;
  }
}

}  // namespace

namespace aspns {

hipError_t launch_debug_shortdiv_wave(int what, unsigned start, unsigned count, unsigned* n_bad, unsigned* bad_bits,
                                      const NsTables* T, hipStream_t s) {
  if (what < 0 || what > 6) return hipErrorInvalidValue;
  hipLaunchKernelGGL(debug_shortdiv_wave_kernel, dim3((count + 255u) / 256u), dim3(256), 0, s, what, start, count,
                     n_bad, bad_bits, T);
  return hipGetLastError();
}

hipError_t launch_debug_fallbacks_wave(int what, unsigned start, unsigned count, unsigned* n_bad, unsigned* bad_bits,
                                       const NsTables* T, hipStream_t s) {
  if (what < 0 || what > 5) return hipErrorInvalidValue;
  hipLaunchKernelGGL(debug_fallbacks_wave_kernel, dim3((count + 255u) / 256u), dim3(256), 0, s, what, start, count,
                     n_bad, bad_bits, T);
  return hipGetLastError();
}

hipError_t launch_debug_guards_wave(unsigned start, unsigned count, unsigned* n_bad, unsigned* bad_bits, hipStream_t s) {
  hipLaunchKernelGGL(debug_guards_wave_kernel, dim3((count + 255u) / 256u), dim3(256), 0, s, start, count, n_bad, bad_bits);
  return hipGetLastError();
}

hipError_t launch_debug_tanh_wave(unsigned start, unsigned count, unsigned* n_bad, unsigned* bad_bits,
                                  const NsTables* T, hipStream_t s) {
  hipLaunchKernelGGL(debug_tanh_wave_kernel, dim3((count + 255u) / 256u), dim3(256), 0, s, start, count, n_bad, bad_bits, T);
  return hipGetLastError();
}

// stamps / step_counts: diagnostics; either one selects the diagnostic kernel (float frames only)
hipError_t launch_ns_frame1(bool io16, float* state, int32_t* hist, const NsTables* T,
                            const float* in, float* out, int num_streams, hipStream_t s, int steady_on,
                            unsigned long long* stamps, int stamp_mode, unsigned* step_counts) {
  const dim3 grid((num_streams + 3) / 4), block(256);
  const NsFlowArgs none = {{nullptr, nullptr}, 0u, 0, 1, 0u, 1u, 1u};
  if (stamps != nullptr || step_counts != nullptr) {
    if (io16) return hipErrorInvalidValue;
    const NsDiagArgs dg = {stamps != nullptr ? (void*)stamps : (void*)step_counts, stamps != nullptr ? (stamp_mode != 0 ? 1 : 0) : 2};
    hipLaunchKernelGGL((ns_frame1_diag_kernel<false>), grid, block, 0, s, state, hist, T, in, out, num_streams,
                       steady_on, none, dg);
  } else if (io16)
    hipLaunchKernelGGL((ns_frame1_kernel<true, false>), grid, block, 0, s, state, hist, T, in, out,
                       num_streams, steady_on, none);
  else
    hipLaunchKernelGGL((ns_frame1_kernel<false, false>), grid, block, 0, s, state, hist, T, in, out,
                       num_streams, steady_on, none);
  return hipGetLastError();
}

// `steps` consecutive frame steps of the hand-off build in one launch: steps want .. want + steps - 1 of every
// stream (seq[s] == want on entry, want + steps on exit, advanced once per walk in between); step j reads / writes
// ring slot (slot0 + j) % ring of in / out (slots `per` floats apart); a workgroup walks `walk` consecutive steps
// (NsFlowArgs).
hipError_t launch_ns_frame1_flow(bool io16, float* state, int32_t* hist, const NsTables* T,
                                 const float* in, float* out, int num_streams, hipStream_t s,
                                 unsigned* seq, unsigned* abort_w, unsigned want, int steps, int walk, int slot0,
                                 int ring, size_t per, int steady_on, unsigned long long* stamps,
                                 unsigned* step_counts) {
  walk = walk < 1 ? 1 : (walk > steps ? steps : walk);
  const int gx = ((num_streams + 3) / 4 + 7) / 8 * 8;
  const dim3 grid(gx, (steps + walk - 1) / walk), block(256);
  const NsFlowArgs fa = {{seq, abort_w}, want, slot0, ring, (unsigned)per, (unsigned)steps, (unsigned)walk};
  if (stamps != nullptr || step_counts != nullptr) {
    if (io16) return hipErrorInvalidValue;
    const NsDiagArgs dg = {stamps != nullptr ? (void*)stamps : (void*)step_counts, stamps != nullptr ? 0 : 2};
    hipLaunchKernelGGL((ns_frame1_diag_kernel<true>), grid, block, 0, s, state, hist, T, in, out, num_streams,
                       steady_on, fa, dg);
  } else if (io16)
    hipLaunchKernelGGL((ns_frame1_kernel<true, true>), grid, block, 0, s, state, hist, T, in, out,
                       num_streams, steady_on, fa);
  else
    hipLaunchKernelGGL((ns_frame1_kernel<false, true>), grid, block, 0, s, state, hist, T, in, out,
                       num_streams, steady_on, fa);
  return hipGetLastError();
}

// The list form: entry i of the n listed streams advances by min(kListMaxSteps, max(0, counts[i] - frame0)) frames;
// in / out point at frame frame0 of [frame][n][160] (`per` floats between two frames); streams / counts: device.
hipError_t launch_ns_frame1_list(bool io16, float* state, int32_t* hist, const NsTables* T, const float* in, float* out,
                                 hipStream_t s, const int32_t* streams, const int32_t* counts, int n,
                                 int frame0, size_t per, int steady_on) {
  if (n < 1) return hipErrorInvalidValue;
  const dim3 grid((n + 3) / 4), block(256);
  const NsFlowArgs fa = {{nullptr, nullptr}, 0u, 0, 1, (unsigned)per, (unsigned)kListMaxSteps, (unsigned)kListMaxSteps};
  const NsListArgs la = {streams, counts, n, frame0};
  if (io16)
    hipLaunchKernelGGL((ns_list1_kernel<true>), grid, block, 0, s, state, hist, T, in, out, steady_on, fa, la);
  else
    hipLaunchKernelGGL((ns_list1_kernel<false>), grid, block, 0, s, state, hist, T, in, out, steady_on, fa, la);
  return hipGetLastError();
}

}  // namespace aspns
