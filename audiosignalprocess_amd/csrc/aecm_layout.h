// aecm_layout.h -- sizes, constant tables and the per-stream work area of the batched mobile echo
// canceller (include/asp_aecm.h), shared by the kernels (aecm_kernels.hip) and the host (aecm_api.hip).
#ifndef ASP_AECM_LAYOUT_H_
#define ASP_AECM_LAYOUT_H_

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "asp_aecm.h"

#if defined(__HIPCC__)
#define AECM_HD __host__ __device__
#else
#define AECM_HD
#endif

namespace aspaecm {

constexpr int kPartLen = 64;                  // PART_LEN
constexpr int kPartLen1 = 65;                 // PART_LEN1
constexpr int kMaxDelay = 100;                // MAX_DELAY: the delay estimator's history
constexpr int kFarBufLen = 256;               // FAR_BUF_LEN
constexpr int kFrameBufLen = 80 + 64;         // FRAME_LEN + PART_LEN: the core's frame rings
constexpr int kFarendBufLen = 50 * 80;        // BUF_SIZE_FRAMES * FRAME_LEN: the far-end ring
constexpr int32_t kMaxBitCountsQ9 = 32 << 9;  // 32 matching bits in Q9
constexpr int kInitCheck = 42;

// Constant tables, built on the host (aecm_api.hip: build_tables) and copied to each device.
struct AecmTables {
  int16_t sin1024[1024];  // kSinTable1024: trunc(32767 sin(2 pi k / 1024))
  int16_t cos360[360];    // WebRtcAecm_kCosTable: trunc(8192 cos(2 pi k / 360)), two entries one lower
  int16_t sin360[360];    // WebRtcAecm_kSinTable: trunc(8192 sin(2 pi k / 360)), four entries adjusted
  int16_t hann[65];       // WebRtcAecm_kSqrtHanning: round(16384 sin(pi k / 129)), k < 64; 16384 at 64
  int16_t ch8[65];        // kChannelStored8kHz: the echo path an 8 kHz instance starts from
  int16_t ch16[65];       // kChannelStored16kHz
};

// One stream's working buffers for a block: the reference keeps them on its stack.  In global memory,
// next to the state, so that the kernel holds no array in private memory.
struct AecmWork {
  int16_t cb[256];                  // the complex FFT buffer (re, im) x 128
  int16_t dfw[130], efw[130];       // near spectrum, and after suppression (re, im) x 65
  uint16_t xfa[65], dfaN[65], dfaC[65];
  int32_t echoEst[65];
  int16_t hnl[65], noiseR[65];
  int16_t farend[80], farFrame[80];
  int16_t blkFar[64], blkNear[64], blkClean[64], outBlock[64];
};

// The echo paths an instance starts from (aecm_core.c: kChannelStored8kHz / kChannelStored16kHz).
static constexpr int16_t kCh8[65] = {2040, 1815, 1590, 1498, 1405, 1395, 1385, 1418, 1451, 1506, 1562, 1644, 1726,
                              1804, 1882, 1918, 1953, 1982, 2010, 2025, 2040, 2034, 2027, 2021, 2014, 1997,
                              1980, 1925, 1869, 1800, 1732, 1683, 1635, 1604, 1572, 1545, 1517, 1481, 1444,
                              1405, 1367, 1331, 1294, 1270, 1245, 1239, 1233, 1247, 1260, 1282, 1303, 1338,
                              1373, 1407, 1441, 1470, 1499, 1524, 1549, 1565, 1582, 1601, 1621, 1649, 1676};
static constexpr int16_t kCh16[65] = {2040, 1590, 1405, 1385, 1451, 1562, 1726, 1882, 1953, 2010, 2040, 2027, 2014,
                               1980, 1869, 1732, 1635, 1572, 1517, 1444, 1367, 1294, 1245, 1233, 1260, 1303,
                               1373, 1441, 1499, 1549, 1582, 1621, 1676, 1741, 1802, 1861, 1921, 1983, 2040,
                               2102, 2170, 2265, 2375, 2515, 2651, 2781, 2922, 3075, 3253, 3471, 3738, 3976,
                               4151, 4258, 4308, 4288, 4270, 4253, 4237, 4179, 4086, 3947, 3757, 3484, 3153};

// The reference's tables are truncated / rounded sines in double precision; the entries where the exact
// value is a multiple of 4096 carry the published table's values.
inline void build_tables(AecmTables* T) {
  for (int k = 0; k < 1024; ++k) T->sin1024[k] = (int16_t)(32767.0 * sin(2.0 * M_PI * k / 1024.0));
  for (int k = 0; k < 360; ++k) {
    T->cos360[k] = (int16_t)(8192.0 * cos(2.0 * M_PI * k / 360.0));
    T->sin360[k] = (int16_t)(8192.0 * sin(2.0 * M_PI * k / 360.0));
  }
  T->cos360[180] = -8191;
  T->cos360[300] = 4095;
  T->sin360[90] = 8191;
  T->sin360[150] = 4096;
  T->sin360[210] = -4095;
  T->sin360[270] = -8191;
  for (int k = 0; k < 64; ++k) T->hann[k] = (int16_t)lround(16384.0 * sin(M_PI * k / 129.0));
  T->hann[64] = 16384;
  memcpy(T->ch8, kCh8, sizeof kCh8);
  memcpy(T->ch16, kCh16, sizeof kCh16);
}

}  // namespace aspaecm
#endif  // ASP_AECM_LAYOUT_H_
