// hpf_core.h -- the high-pass filter's arithmetic (high_pass_filter_impl.cc's InitializeFilter and Filter), one
// source for the kernel (hpf_kernels.hip) and the CPU build (hpf_restate.cpp).
//
// The filter state lives in int32 registers that hold int16 values.  Every sum is taken on uint32_t: none of them
// leaves int32 on any input (the worst case is pinned by the golden), so this is the reference's arithmetic, and
// where the reference shifts a negative value left (y[0] << 13, the << 1 and << 2) it is what gcc computes.
// The cast to y[0] does wrap once the filter's output passes about twice full scale; i16() is that cast.
#ifndef ASP_HPF_CORE_H_
#define ASP_HPF_CORE_H_

#include <stdint.h>

#include "hpf_layout.h"

namespace asphpf {

HPF_HD inline int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
HPF_HD inline int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
HPF_HD inline int32_t wshl(int32_t a, int s) { return (int32_t)((uint32_t)a << s); }
// the product of two values that fit 24 bits (samples, state words and coefficients fit 16): one full-rate
// v_mul_i32_i24 / v_mad_i32_i24 on the device instead of a quarter-rate 32-bit multiply, the same 32 bits
HPF_HD inline int32_t mul16(int32_t a, int32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(a, b);
#else
  return a * b;
#endif
}
HPF_HD inline int32_t i16(int32_t v) { return (int32_t)(int16_t)(uint16_t)(uint32_t)v; }

// ba: {b0, b1, b2, -a1, -a2} in Q12 (kFilterCoefficients8kHz, kFilterCoefficients)
struct HpfCoeffs {
  int32_t b0, b1, b2, a1, a2;
};

HPF_HD inline HpfCoeffs coeffs(int set) {
  return set == 0 ? HpfCoeffs{3798, -7596, 3798, 7807, -3733} : HpfCoeffs{4012, -8024, 4012, 8002, -3913};
}

// the coefficient set InitializeFilter picks, or -1 for a rate the audio processing module does not run at
HPF_HD inline int coeff_set_of_rate(int sample_rate_hz) {
  if (sample_rate_hz == 8000) return 0;
  return sample_rate_hz == 16000 || sample_rate_hz == 32000 || sample_rate_hz == 48000 ? 1 : -1;
}

struct HpfRegs {
  int32_t y0, y1, y2, y3, x0, x1;
};

HPF_HD inline HpfRegs load_regs(const AspHpfState& s) { return HpfRegs{s.y[0], s.y[1], s.y[2], s.y[3], s.x[0], s.x[1]}; }
HPF_HD inline void store_regs(AspHpfState& s, const HpfRegs& r) {
  s.y[0] = (int16_t)r.y0;
  s.y[1] = (int16_t)r.y1;
  s.y[2] = (int16_t)r.y2;
  s.y[3] = (int16_t)r.y3;
  s.x[0] = (int16_t)r.x0;
  s.x[1] = (int16_t)r.x1;
}

// One sample of Filter.  The feed-forward sum and everything after the state update hang off the feedback chain
// (y1, y0 -> t -> y0 -> y1) and are left for the scheduler to place under it.
HPF_HD inline int32_t filter_sample(HpfRegs& r, const HpfCoeffs& c, int32_t d) {
  const int32_t ff = wadd(wadd(mul16(d, c.b0), mul16(r.x0, c.b1)), mul16(r.x1, c.b2));
  int32_t t = wadd(mul16(r.y1, c.a1), mul16(r.y3, c.a2)) >> 15;
  t = wadd(t, wadd(mul16(r.y0, c.a1), mul16(r.y2, c.a2)));
  t = wadd(wshl(t, 1), ff);
  r.x1 = r.x0;
  r.x0 = d;
  r.y2 = r.y0;
  r.y3 = r.y1;
  r.y0 = i16(t >> 13);
  r.y1 = i16(wshl(wsub(t, wshl(r.y0, 13)), 2));
  t = wadd(t, 2048);
  t = t > 134217727 ? 134217727 : t < -134217728 ? -134217728 : t;
  return t >> 12;   // within int16 after the clamp
}

HPF_HD inline void init_state(AspHpfState& s, int coeff_set) {
  s = AspHpfState{{0, 0, 0, 0}, {0, 0}, (int16_t)coeff_set, 0};
}

}  // namespace asphpf

#endif  // ASP_HPF_CORE_H_
