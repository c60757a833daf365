// nsx_layout.h -- constant tables and the per-stream work area of the batched fixed-point noise
// suppressor (include/asp_nsx.h), shared by the kernels (nsx_kernels.hip), the host (nsx_api.hip) and
// the CPU build of the core (nsx_restate.cpp).
#ifndef ASP_NSX_LAYOUT_H_
#define ASP_NSX_LAYOUT_H_

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "asp_nsx.h"

#if defined(__HIPCC__)
#define NSX_HD __host__ __device__
#else
#define NSX_HD
#endif

namespace aspnsx {

constexpr int kStartBand = 5;
constexpr int kHist = 1000;  // HIST_PAR_EST

// Constant tables, built on the host (build_tables) and copied to each device.
struct NsxTables {
  int16_t sin1024[1024];     // kSinTable1024: trunc(32767 sin(2 pi k / 1024))
  int16_t win128[128];       // kBlocks80w128x: 48-sample sine flanks round(16384 sin(pi k / 96)), flat between
  int16_t win256[256];       // kBlocks160w256x: 96-sample flanks round(16384 sin(pi k / 192))
  int16_t logFrac[256];      // kLogTableFrac: round(256 log2(1 + k / 256))
  int16_t counterDiv[201];   // kCounterDiv: round(32768 / (k + 1)), at most 32767
  int16_t logTable[9];       // kLogTable: round(256 k ln 2)
  int16_t logIndex[129];     // kLogIndex: round(4096 log2 k), 0 at k = 0
  int16_t sumLogIndex[66];   // kSumLogIndex: round(32 sum_{j=k}^{128} log2 j), 0 at k = 0
  int16_t sumSqLogIndex[66]; // kSumSquareLogIndex: round(4 sum_{j=k}^{128} log2(j)^2)
  int16_t detEstMatrix[66];  // kDeterminantEstMatrix: round((129 - k) sum log2(j)^2 - (sum log2 j)^2)
  int16_t factor1[257];      // kFactor1Table: trunc(8192 f1(sqrt(k / 256)))
  int16_t factor2[3][257];   // kFactor2Aggressiveness1..3: trunc(8192 f2(sqrt(k / 256), bound))
  int16_t indicator[17];     // kIndicatorTable
};

// One stream's working arrays for a frame (the reference keeps them on its stack).  In LDS on the GPU.
struct NsxWork {
  int16_t cb[512];      // the complex FFT buffer (re, im) x 256
  int16_t win[256];     // windowed input; scratch of the buffer shifts
  uint16_t magn[129], prevNoiseU16[129], nsp[129], filtTmp[129];
  int16_t lmagn[129];
  uint32_t noise[129], postSnr[129], priorSnr[129], prevNearSnr[129];
};

static constexpr int16_t kIndicator[17] = {0,    2017, 3809, 5227, 6258, 6963, 7424, 7718, 7901,
                                           8014, 8084, 8126, 8152, 8168, 8177, 8183, 8187};

inline void build_tables(NsxTables* T) {
  for (int k = 0; k < 1024; ++k) T->sin1024[k] = (int16_t)(32767.0 * sin(2.0 * M_PI * k / 1024.0));
  for (int k = 0; k < 128; ++k) {
    const int d = k < 48 ? k : k <= 80 ? 48 : 128 - k;
    T->win128[k] = (int16_t)floor(16384.0 * sin(M_PI * d / 96.0) + 0.5);
  }
  for (int k = 0; k < 256; ++k) {
    const int d = k < 96 ? k : k <= 160 ? 96 : 256 - k;
    T->win256[k] = (int16_t)floor(16384.0 * sin(M_PI * d / 192.0) + 0.5);
  }
  for (int k = 0; k < 256; ++k) T->logFrac[k] = (int16_t)floor(256.0 * log2(1.0 + k / 256.0) + 0.5);
  for (int k = 0; k < 201; ++k) {
    const double v = floor(32768.0 / (k + 1) + 0.5);
    T->counterDiv[k] = (int16_t)(v > 32767.0 ? 32767.0 : v);
  }
  for (int k = 0; k < 9; ++k) T->logTable[k] = (int16_t)floor(k * log(2.0) * 256.0 + 0.5);
  T->logIndex[0] = 0;
  for (int k = 1; k < 129; ++k) T->logIndex[k] = (int16_t)floor(4096.0 * log2((double)k) + 0.5);
  T->sumLogIndex[0] = T->sumSqLogIndex[0] = T->detEstMatrix[0] = 0;
  for (int k = 1; k < 66; ++k) {
    double s = 0.0, q = 0.0;
    for (int j = k; j < 129; ++j) {
      const double l = log2((double)j);
      s += l;
      q += l * l;
    }
    T->sumLogIndex[k] = (int16_t)floor(32.0 * s + 0.5);
    T->sumSqLogIndex[k] = (int16_t)floor(4.0 * q + 0.5);
    T->detEstMatrix[k] = (int16_t)floor((129 - k) * q - s * s + 0.5);
  }
  // gain-compensation factors over the energy ratio in Q8: g = sqrt(k / 256), B_LIM = 0.5
  static const double bound[3] = {0.25, 0.125, 0.09};
  for (int k = 0; k < 257; ++k) {
    const double g = sqrt(k / 256.0);
    double f1 = 1.0;
    if (g > 0.5) {
      f1 = 1.0 + 1.3 * (g - 0.5);
      if (g * f1 > 1.0) f1 = 1.0 / g;
    }
    T->factor1[k] = (int16_t)(8192.0 * f1);
    for (int a = 0; a < 3; ++a) {
      const double gg = g > bound[a] ? g : bound[a];
      T->factor2[a][k] = (int16_t)(g < 0.5 ? 8192.0 * (1.0 - 0.3 * (0.5 - gg)) : 8192.0);
    }
  }
  memcpy(T->indicator, kIndicator, sizeof kIndicator);
}

}  // namespace aspnsx
#endif  // ASP_NSX_LAYOUT_H_
