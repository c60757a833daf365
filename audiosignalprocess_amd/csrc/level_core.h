// level_core.h -- RMSLevel's arithmetic (rms_level.cc), one source for the kernel (level_kernels.hip), the host
// side of the C ABI (level_api.hip: RMS() is evaluated on the host) and the CPU build (hpf_restate.cpp).
//
// Process: the int product of a sample with itself, converted to float, one float add per sample in sample order.
// Past 2^24 the sum rounds at every add, so the order is part of the result: nothing here may be reassociated.
#ifndef ASP_LEVEL_CORE_H_
#define ASP_LEVEL_CORE_H_

#include <math.h>
#include <stdint.h>

#include "hpf_layout.h"

namespace asphpf {

HPF_HD inline void level_add(float& sum_square, int32_t d) { sum_square += (float)(d * d); }

HPF_HD inline void level_count(AspLevelState& s, int32_t length) {
  s.sample_count = (int32_t)((uint32_t)s.sample_count + (uint32_t)length);
}

// RMSLevel::RMS() as written: the float division, log10 on a float, (int)(rms + 0.5); resets the state.  Host only.
inline int level_rms(AspLevelState& s) {
  const float kMaxSquaredLevel = 32768 * 32768;
  const int kMinLevel = ASP_LEVEL_MIN;
  const float sum_square = s.sum_square;
  const int sample_count = s.sample_count;
  s.sum_square = 0;
  s.sample_count = 0;
  if (sample_count == 0 || sum_square == 0) return kMinLevel;
  float rms = sum_square / (sample_count * kMaxSquaredLevel);
  rms = 10 * log10(rms);
  if (rms < -kMinLevel) rms = -kMinLevel;
  rms = -rms;
  return static_cast<int>(rms + 0.5);
}

}  // namespace asphpf

#endif  // ASP_LEVEL_CORE_H_
