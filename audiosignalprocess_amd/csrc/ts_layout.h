// ts_layout.h -- sizes, the per-batch configuration, the table set and the work memory of the transient
// suppressor (ts_core.h).  Shared by the kernel, the host API and the CPU build.
#ifndef ASP_TS_LAYOUT_H_
#define ASP_TS_LAYOUT_H_

#include <stdint.h>

#include "asp_ts.h"

namespace aspts {

constexpr int kMaxN = 1024;            // analysis length at 48 kHz
constexpr int kMaxBins = kMaxN / 2 + 1;
constexpr int kMaxDet = 480;           // detection chunk at 48 kHz
constexpr int kLeaves = ASP_TS_LEAVES;
constexpr int kTaps = 16;              // Daubechies 8: 16 coefficients
constexpr int kHist = ASP_TS_HISTORY;
constexpr int kMaxLeaf = kMaxDet / kLeaves;
constexpr int kPhases = 32768;         // WebRtcSpl_RandU's range
constexpr int kMinVoiceBin = 3, kMaxVoiceBin = 60;

// transient_suppressor.cc:68-116 and transient_detector.cc:30-48
struct TsConfig {
  int rate, det_rate, C;
  int N, L, delay, bins;  // analysis_length_, data_length_, buffer_delay_, complex_analysis_length_
  int D, T;               // detection_length_, tree_leaves_data_length_ (the moment queues hold 3 T)
};

// Create-time tables in device (kernel) or host (CPU build) memory
struct TsTables {
  const float* window;       // [N]
  const float* w;            // [N / 2]: makewt(N / 4) then makect(N / 4)
  const float* mean_factor;  // [bins]
  const float* phase;        // [kPhases][2]: cosf, sinf of 2 * kPi * r / 32767
};

// tree: the node arrays of the three upper levels, each [15 history][data], then the leaves
constexpr int kTreeFloats = (kHist + kMaxDet) + 2 * kHist + kMaxDet + 4 * kHist + kMaxDet + kMaxDet;

struct TsWork {
  union {
    struct {
      float fb[kMaxN + 2];  // fft_buffer_
      float xb[kMaxN];      // staging of a shifted buffer
    } s;
    float tree[kTreeFloats];
  };
  float mag[kMaxBins + 3];  // magnitudes_
  float m1[kLeaves][kMaxLeaf], m2[kLeaves][kMaxLeaf];  // first_moments_, second_moments_ of every leaf
  float term[kMaxDet];
  int32_t cnt[64 + 1];
  float scal[4];
};

static_assert(sizeof(((TsWork*)0)->s) >= sizeof(float) * kTreeFloats, "the tree shares the transform's buffers");

// floats of a stream's buffer array: in [C][N], out [C][N], mean [C][bins]
inline size_t buffer_floats(const TsConfig& c) { return (size_t)c.C * (2 * c.N + c.bins); }

}  // namespace aspts
#endif  // ASP_TS_LAYOUT_H_
