// bf_layout.h -- sizes, the per-batch parameters, the table set and the work memory of the beamformer
// (bf_core.h).  Shared by the kernel, the host API and the CPU build.
#ifndef ASP_BF_LAYOUT_H_
#define ASP_BF_LAYOUT_H_

#include <stdint.h>

#include "asp_bf.h"

namespace aspbf {

constexpr int kFft = 256;                  // Beamformer::kFftSize
constexpr int kBins = ASP_BF_BINS;         // kNumFreqBins
constexpr int kChunk = ASP_BF_CHUNK;       // chunk_length_ at 16 kHz, 10 ms
constexpr int kShift = kFft / 2;           // the lapped transform's shift
constexpr int kDelay = 224;                // Blocker::initial_delay_ = 256 - gcd(160, 128)
constexpr int kBuf = ASP_BF_BUFFER;        // chunk + initial delay
constexpr int kMinM = ASP_BF_MIN_MICS, kMaxM = ASP_BF_MAX_MICS;
constexpr int kMedianIx = (kBins + 1) / 2;  // EstimateTargetPresence's order statistic: 65
constexpr float kMaskMinimum = 0.01f;
constexpr float kMaskTargetThreshold = 0.3f;

// the Initialize-time tables of include/asp_bf.h, in its numbering
enum { kTabWindow, kTabWave, kTabThr, kTabDsm, kTabTcov, kTabIcov, kTabRxiw, kTabRpsiw, kTabRrpsiw, kTabDecay, kTabCount };

inline int table_length(int which, int M) {
  switch (which) {
    case kTabWindow: return kFft;
    case kTabDsm: return kBins * M * 2;
    case kTabTcov:
    case kTabIcov: return kBins * M * M * 2;
    case kTabDecay: return 1;
    default: return which >= 0 && which < kTabCount ? kBins : -1;
  }
}

// Beamformer::Initialize's scalars (beamformer.cc:139-161)
struct BfParams {
  int M;
  float decay;                            // decay_threshold_
  int mid_lo, mid_hi, high_lo, high_hi;   // the bin bounds: 4, 6, 64, 112 at 16 kHz
  int hold;                               // hold_target_blocks_: 31
};

// The tables as the kernel reads them, one float array in device (kernel) or host (CPU build) memory.  The
// matrices are bin-minor so that lanes on consecutive bins read consecutive complex values:
// dsm [M][129][2], tcov and icov [M * M][129][2] with element (row j, column i) at j * M + i.
struct BfTables {
  const float* window;  // [256]
  const float* w;       // [128]: ts_core.h's make_fft_w(256)
  const float* thr;     // [129]
  const float* rxiw;    // [129]
  const float* rpsiw;   // [129]
  const float* rrpsiw;  // [129]
  const float* dsm;
  const float* tcov;
  const float* icov;
};

constexpr int kPackFixed = kFft + kFft / 2 + 4 * kBins;  // window, w, thr, rxiw, rpsiw, rrpsiw
inline int pack_floats(int M) { return kPackFixed + 2 * kBins * (M + 2 * M * M); }
inline BfTables view_tables(const float* p, int M) {
  BfTables t;
  t.window = p;
  t.w = p + kFft;
  t.thr = t.w + kFft / 2;
  t.rxiw = t.thr + kBins;
  t.rpsiw = t.rxiw + kBins;
  t.rrpsiw = t.rpsiw + kBins;
  t.dsm = t.rrpsiw + kBins;
  t.tcov = t.dsm + 2 * kBins * M;
  t.icov = t.tcov + 2 * kBins * M * M;
  return t;
}

// A stream's work memory apart from its state: LDS on the device.  spec: the M windowed blocks, transformed in
// place (rdft's packing); ob: the output block.
struct BfScalars {
  float median, old_high;
  int nblocks;
};
template <int M>
struct BfWork {
  float spec[M][kFft];
  float ob[kFft];
  float ramp[kChunk];
  BfScalars sc;
};

// floats of a stream's buffer array: the input buffer [M][384], the output buffer [384]
inline size_t buffer_floats(int M) { return (size_t)(M + 1) * kBuf; }

}  // namespace aspbf
#endif  // ASP_BF_LAYOUT_H_
