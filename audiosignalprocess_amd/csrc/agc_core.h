// agc_core.h -- the legacy gain control (include/asp_agc.h) restated once: analog_agc.c, digital_agc.c and
// the spl primitives they use (DownsampleBy2, DotProductWithScale, DivW32W16, DivW32W16ResW16, Sqrt,
// NormW32, NormU32, AddSatW16), compiled as __device__ code by agc_kernels.hip, as host code by agc_api.hip
// (Init, set_config) and into lib/libagc_restate.so by agc_restate.cpp (tests only).
//
// A stream is served by a group of W lanes (Grp<W>): 16 on the GPU, 1 on the CPU.  Per-sample work (the
// sub-frame envelope maxima, the AddMic / VirtualMic gains, the block energies, the gain ramp over the
// bands) strides over the group; the serial parts sit on single lanes of it: the three AgcVad chains run as
// one pass on lanes 0..2 (one loop, each lane on its own state and input), AddMic's by-2 decimator is a
// second pass on lane 3, the capacitor recurrences and ProcessAnalog run on lane 0, the limiter loop one
// sub-frame per lane.  wsync() separates the sections.
//
// Kept from the reference bit for bit: AddMic's energy loop decimates only at fs == 16000; only the first
// sub-frame of the gain ramp has the clip test; the /256*253 against *253/256 split of the limiter loop; the
// > 8388608 split of the gate; VirtualMic's table index after a clip (gainIdx - 127 against - 128); scale
// is 0; Process skips ProcessAnalog for a low-level signal in adaptive-digital mode.  Where the reference
// relies on 32-bit wrap-around (gain32 *= gain32, shifts of negative values, the AgcVad energy) the code
// below does two's-complement arithmetic on uint32_t (wadd / wsub / wmul / wshl); the golden's reference
// build uses -fwrapv, which defines the same.
//
// Not in the reference: table and ring indices are clamped to their arrays (they are in range for every
// state the entry points can produce), and a division whose reference divisor would be 0 yields 0.
//
// Fields WebRtcAgc_Init does not write (Rxx16w32_array[1], inActive's neighbours, lastError, ...) keep what
// malloc gave the reference; here a state is all zero after Create, and the golden's generator zeroes the
// reference's struct before Init for the same reason.
#ifndef ASP_AGC_CORE_H_
#define ASP_AGC_CORE_H_

#include <stdint.h>
#include <string.h>

#include "agc_layout.h"

namespace aspagc {

// ------------------------------------------------------------------ lanes
template <int W>
struct Grp;
template <>
struct Grp<1> {
  int lane;
  AGC_HD int32_t max(int32_t v) const { return v; }
  AGC_HD int32_t sum(int32_t v) const { return v; }
  AGC_HD bool is(int) const { return true; }
};
#if defined(__HIPCC__)
template <>
struct Grp<16> {
  int lane;
  __device__ int32_t max(int32_t v) const {
    for (int m = 8; m > 0; m >>= 1) {
      const int32_t o = __shfl_xor(v, m, 16);
      v = o > v ? o : v;
    }
    return v;
  }
  __device__ int32_t sum(int32_t v) const {   // wrap-around sum, any order gives the same bits
    for (int m = 8; m > 0; m >>= 1) v = (int32_t)((uint32_t)v + (uint32_t)__shfl_xor(v, m, 16));
    return v;
  }
  __device__ bool is(int k) const { return lane == k; }
};
#endif

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#else
AGC_HD inline void wsync() {}
#endif

// ------------------------------------------------------------------ arithmetic
AGC_HD inline int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
AGC_HD inline int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
AGC_HD inline int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
AGC_HD inline int32_t wshl(int32_t a, int n) { return n > 31 ? 0 : (int32_t)((uint32_t)a << n); }
AGC_HD inline int32_t shift_w32(int32_t x, int c) { return c >= 0 ? wshl(x, c) : x >> (-c > 31 ? 31 : -c); }
AGC_HD inline int16_t sat16(int32_t v) { return (int16_t)(v > 32767 ? 32767 : v < -32768 ? -32768 : v); }
AGC_HD inline int16_t add_sat_w16(int16_t a, int16_t b) { return sat16((int32_t)a + b); }
AGC_HD inline int32_t div_w32w16(int32_t num, int16_t den) { return den != 0 ? num / den : 0x7FFFFFFF; }
AGC_HD inline int16_t div_w32w16_res16(int32_t num, int16_t den) { return den != 0 ? (int16_t)(num / den) : (int16_t)0x7FFF; }
AGC_HD inline int clz_steps(uint32_t a, uint32_t m16, uint32_t m8, uint32_t m4, uint32_t m2, uint32_t m1) {
  int z = (m16 & a) ? 0 : 16;
  if (!(m8 & (a << z))) z += 8;
  if (!(m4 & (a << z))) z += 4;
  if (!(m2 & (a << z))) z += 2;
  if (!(m1 & (a << z))) z += 1;
  return z;
}
AGC_HD inline int16_t norm_w32(int32_t a) {
  if (a == 0) return 0;
  if (a < 0) a = ~a;
  return (int16_t)clz_steps((uint32_t)a, 0xFFFF8000u, 0xFF800000u, 0xF8000000u, 0xE0000000u, 0xC0000000u);
}
AGC_HD inline int16_t norm_u32(uint32_t a) {
  if (a == 0) return 0;
  return (int16_t)clz_steps(a, 0xFFFF0000u, 0xFF000000u, 0xF0000000u, 0xC0000000u, 0x80000000u);
}
// C + (B >> 16) * A + (((B & 0xFFFF) * A) >> 16): the spl form is unsigned in its last term, the AGC form signed
AGC_HD inline int32_t spl_scalediff32(uint16_t A, int32_t B, int32_t C) {
  return (int32_t)((uint32_t)C + (uint32_t)wmul(B >> 16, A) + (((uint32_t)(0xFFFF & B) * A) >> 16));
}
AGC_HD inline int32_t agc_scalediff32(int32_t A, int32_t B, int32_t C) {
  return wadd(wadd(C, wmul(B >> 16, A)), wmul(0xFFFF & B, A) >> 16);
}
AGC_HD inline int32_t agc_mul32(int32_t A, int32_t B) { return wadd(wmul(B >> 13, A), wmul(0x1FFF & B, A) >> 13); }

AGC_HD inline int32_t sqrt_local(int32_t in) {
  int32_t B = in / 2;
  B = wsub(B, 0x40000000);
  const int16_t x_half = (int16_t)(B >> 16);
  B = wadd(B, 0x40000000);
  B = wadd(B, 0x40000000);
  const int32_t x2 = wmul(wmul(x_half, x_half), 2);
  int32_t A = wsub(0, x2);
  B = wadd(B, A >> 1);
  A >>= 16;
  A = wmul(wmul(A, A), 2);
  int16_t t16 = (int16_t)(A >> 16);
  B = wadd(B, wmul(-20480 * t16, 2));
  A = wmul(x_half * t16, 2);
  t16 = (int16_t)(A >> 16);
  B = wadd(B, wmul(28672 * t16, 2));
  t16 = (int16_t)(x2 >> 16);
  A = wmul(x_half * t16, 2);
  B = wadd(B, A >> 1);
  return wadd(B, 32768);
}
AGC_HD inline int32_t spl_sqrt(int32_t value) {
  int32_t A = value;
  if (A == 0) return 0;
  const int16_t sh = norm_w32(A);
  A = wshl(A, sh);
  A = A < 0x7FFFFFFF - 32767 ? wadd(A, 32768) : 0x7FFFFFFF;
  const int16_t x_norm = (int16_t)(A >> 16);
  const int16_t nshift = sh / 2;
  A = wshl(x_norm, 16);
  A = A >= 0 ? A : wsub(0, A);
  A = sqrt_local(A);
  if (2 * nshift == sh) {
    const int16_t t16 = (int16_t)(A >> 16);
    A = wmul(23170 * t16, 2);
    A = wadd(A, 32768);
    A &= 0x7fff0000;
    A >>= 15;
  } else {
    A >>= 16;
  }
  A &= 0xffff;
  return A >> nshift;
}

// WebRtcSpl_DownsampleBy2, one output per call: the two all-pass branches on samples a (lower) and b (upper)
struct Ds2 {
  int32_t s0, s1, s2, s3, s4, s5, s6, s7;
};
AGC_HD inline Ds2 ds2_load(const int32_t* p) { return Ds2{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]}; }
AGC_HD inline void ds2_store(int32_t* p, const Ds2& d) {
  p[0] = d.s0; p[1] = d.s1; p[2] = d.s2; p[3] = d.s3; p[4] = d.s4; p[5] = d.s5; p[6] = d.s6; p[7] = d.s7;
}
AGC_HD inline int16_t ds2_step(Ds2& d, int16_t a, int16_t b) {
  int32_t in32 = (int32_t)a * 1024;
  int32_t diff = wsub(in32, d.s1);
  int32_t tmp1 = spl_scalediff32(12199, diff, d.s0);
  d.s0 = in32;
  diff = wsub(tmp1, d.s2);
  int32_t tmp2 = spl_scalediff32(37471, diff, d.s1);
  d.s1 = tmp1;
  diff = wsub(tmp2, d.s3);
  d.s3 = spl_scalediff32(60255, diff, d.s2);
  d.s2 = tmp2;
  in32 = (int32_t)b * 1024;
  diff = wsub(in32, d.s5);
  tmp1 = spl_scalediff32(3284, diff, d.s4);
  d.s4 = in32;
  diff = wsub(tmp1, d.s6);
  tmp2 = spl_scalediff32(24441, diff, d.s5);
  d.s5 = tmp1;
  diff = wsub(tmp2, d.s7);
  d.s7 = spl_scalediff32(49528, diff, d.s6);
  d.s6 = tmp2;
  return sat16(wadd(wadd(d.s3, d.s7), 1024) >> 11);
}

// ------------------------------------------------------------------ AgcVad
struct VadRef {
  int32_t* downState;
  int16_t *HPstate, *counter, *logRatio, *meanLongTerm;
  int32_t* varianceLongTerm;
  int16_t *stdLongTerm, *meanShortTerm;
  int32_t* varianceShortTerm;
  int16_t* stdShortTerm;
};
#define AGC_VAD(s, p)                                                                                         \
  VadRef {                                                                                                    \
    (s).p##_downState, &(s).p##_HPstate, &(s).p##_counter, &(s).p##_logRatio, &(s).p##_meanLongTerm,          \
        &(s).p##_varianceLongTerm, &(s).p##_stdLongTerm, &(s).p##_meanShortTerm, &(s).p##_varianceShortTerm, \
        &(s).p##_stdShortTerm                                                                                 \
  }

AGC_HD inline void init_vad(VadRef v) {
  *v.HPstate = 0;
  *v.logRatio = 0;
  *v.meanLongTerm = 15 << 10;
  *v.varianceLongTerm = 500 << 8;
  *v.stdLongTerm = 0;
  *v.meanShortTerm = 15 << 10;
  *v.varianceShortTerm = 500 << 8;
  *v.stdShortTerm = 0;
  *v.counter = 3;
  for (int k = 0; k < 8; ++k) v.downState[k] = 0;
}

// WebRtcAgc_ProcessVad on n = 80 or 160 samples
AGC_HD inline int16_t process_vad(VadRef v, const int16_t* in, int n) {
  int32_t nrg = 0;
  int16_t hp = *v.HPstate;
  Ds2 d = ds2_load(v.downState);
  const bool wide = n == 160;
  for (int j = 0; j < 40; ++j) {   // 10 sub-frames of 4 samples at 4 kHz
    int16_t a, b;
    if (wide) {
      a = (int16_t)(((int32_t)in[4 * j] + in[4 * j + 1]) >> 1);
      b = (int16_t)(((int32_t)in[4 * j + 2] + in[4 * j + 3]) >> 1);
    } else {
      a = in[2 * j];
      b = in[2 * j + 1];
    }
    const int16_t x = ds2_step(d, a, b);
    const int32_t out = x + hp;
    hp = (int16_t)(((600 * out) >> 10) - x);
    nrg = wadd(nrg, wmul(out, out) >> 6);
  }
  ds2_store(v.downState, d);
  *v.HPstate = hp;

  const int zeros = clz_steps((uint32_t)nrg, 0xFFFF0000u, 0xFF000000u, 0xF0000000u, 0xC0000000u, 0x80000000u);
  const int16_t dB = (int16_t)((15 - zeros) * 2048);
  if (*v.counter < 250) ++*v.counter;
  const int16_t counter = *v.counter;

  int32_t t = *v.meanShortTerm * 15 + dB;
  *v.meanShortTerm = (int16_t)(t >> 4);
  t = (dB * dB) >> 12;
  t = wadd(t, wmul(*v.varianceShortTerm, 15));
  *v.varianceShortTerm = t / 16;
  t = *v.meanShortTerm * *v.meanShortTerm;
  t = wsub(wshl(*v.varianceShortTerm, 12), t);
  *v.stdShortTerm = (int16_t)spl_sqrt(t);

  t = *v.meanLongTerm * counter + dB;
  *v.meanLongTerm = div_w32w16_res16(t, add_sat_w16(counter, 1));
  t = (dB * dB) >> 12;
  t = wadd(t, wmul(*v.varianceLongTerm, counter));
  *v.varianceLongTerm = div_w32w16(t, add_sat_w16(counter, 1));
  t = *v.meanLongTerm * *v.meanLongTerm;
  t = wsub(wshl(*v.varianceLongTerm, 12), t);
  *v.stdLongTerm = (int16_t)spl_sqrt(t);

  t = 12288 * (int16_t)(dB - *v.meanLongTerm);
  t = div_w32w16(t, *v.stdLongTerm);
  const int32_t tb = *v.logRatio * 53248;
  t = wadd(t, tb >> 10);
  int16_t lr = (int16_t)(t >> 6);
  if (lr > 2048) lr = 2048;
  if (lr < -2048) lr = -2048;
  *v.logRatio = lr;
  return lr;
}

// ------------------------------------------------------------------ digital_agc.c
// WebRtcAgc_CalculateGainTable
AGC_HD inline int32_t calculate_gain_table(int32_t* gainTable, int16_t digCompGaindB, int16_t targetLevelDbfs,
                                           uint8_t limiterEnable, int16_t analogTarget) {
  const int32_t kLog10 = 54426, kLog10_2 = 49321, kLogE_1 = 23637;
  const int16_t kCompRatio = 3;
  int32_t tmp32no1 = (digCompGaindB - analogTarget) * (kCompRatio - 1);
  int16_t tmp16no1 = (int16_t)(analogTarget - targetLevelDbfs);
  tmp16no1 = (int16_t)(tmp16no1 + div_w32w16_res16(tmp32no1 + (kCompRatio >> 1), kCompRatio));
  const int16_t maxGain = (int16_t)(tmp16no1 > analogTarget - targetLevelDbfs ? tmp16no1 : analogTarget - targetLevelDbfs);
  // (zeroGainLvl of the reference is computed and never read)
  tmp32no1 = digCompGaindB * (kCompRatio - 1);
  const int16_t diffGain = div_w32w16_res16(tmp32no1 + (kCompRatio >> 1), kCompRatio);
  if (diffGain < 0 || diffGain >= 128) return -1;
  const int16_t limiterLvlX = analogTarget;  // limiterOffset is 0
  const int16_t limiterIdx = (int16_t)(2 + div_w32w16_res16(wshl(limiterLvlX, 13), (int16_t)(kLog10_2 / 2)));
  const int32_t limiterLvl = targetLevelDbfs + div_w32w16_res16(kCompRatio >> 1, kCompRatio);
  const uint16_t constMaxGain = kGenFuncTable[diffGain];
  const int16_t constLinApprox = 22817;
  const int32_t den = 20 * (int32_t)constMaxGain;
  for (int16_t i = 0; i < 32; i++) {
    int16_t tmp16 = (int16_t)((kCompRatio - 1) * (i - 1));
    int32_t tmp32 = tmp16 * kLog10_2 + 1;
    int32_t inLevel = div_w32w16(tmp32, kCompRatio);
    inLevel = ((int32_t)diffGain << 14) - inLevel;
    const uint32_t absInLevel = (uint32_t)(inLevel >= 0 ? inLevel : -inLevel);
    uint16_t intPart = (uint16_t)(absInLevel >> 14);
    uint16_t fracPart = (uint16_t)(absInLevel & 0x3FFF);
    const int lo = intPart > 127 ? 127 : intPart, hi = intPart + 1 > 127 ? 127 : intPart + 1;
    const uint16_t tmpU16 = (uint16_t)(kGenFuncTable[hi] - kGenFuncTable[lo]);
    uint32_t tmpU32no1 = (uint32_t)tmpU16 * fracPart;
    tmpU32no1 += (uint32_t)kGenFuncTable[lo] << 14;
    uint32_t logApprox = tmpU32no1 >> 8;
    if (inLevel < 0) {
      const int zeros = norm_u32(absInLevel);
      int zerosScale = 0;
      uint32_t tmpU32no2;
      if (zeros < 15) {
        tmpU32no2 = absInLevel >> (15 - zeros);
        tmpU32no2 = tmpU32no2 * (uint32_t)kLogE_1;
        if (zeros < 9) {
          zerosScale = 9 - zeros;
          tmpU32no1 >>= zerosScale;
        } else {
          tmpU32no2 >>= zeros - 9;
        }
      } else {
        tmpU32no2 = absInLevel * (uint32_t)kLogE_1;
        tmpU32no2 >>= 6;
      }
      logApprox = 0;
      if (tmpU32no2 < tmpU32no1) logApprox = (tmpU32no1 - tmpU32no2) >> (8 - zerosScale);
    }
    int32_t numFIX = wshl(maxGain * (int32_t)constMaxGain, 6);
    numFIX = wsub(numFIX, wmul((int32_t)logApprox, diffGain));
    int zeros;
    if (numFIX > (den >> 8))
      zeros = norm_w32(numFIX);
    else
      zeros = norm_w32(den) + 8;
    numFIX = wshl(numFIX, zeros);
    tmp32no1 = shift_w32(den, zeros - 8);
    if (numFIX < 0)
      numFIX = wsub(numFIX, tmp32no1 / 2);
    else
      numFIX = wadd(numFIX, tmp32no1 / 2);
    int32_t y32 = tmp32no1 != 0 ? numFIX / tmp32no1 : 0;
    if (limiterEnable && (i < limiterIdx)) {
      tmp32 = (int16_t)(i - 1) * kLog10_2;
      tmp32 = wsub(tmp32, wshl(limiterLvl, 14));
      y32 = div_w32w16(wadd(tmp32, 10), 20);
    }
    if (y32 > 39000) {
      tmp32 = wadd(wmul(y32 >> 1, kLog10), 4096);
      tmp32 >>= 13;
    } else {
      tmp32 = wadd(wmul(y32, kLog10), 8192);
      tmp32 >>= 14;
    }
    tmp32 = wadd(tmp32, 16 << 14);
    if (tmp32 > 0) {
      intPart = (uint16_t)(int16_t)(tmp32 >> 14);
      fracPart = (uint16_t)(tmp32 & 0x3FFF);
      int32_t tmp32no2;
      if ((fracPart >> 13) != 0) {
        tmp16 = (int16_t)((2 << 14) - constLinApprox);
        tmp32no2 = (1 << 14) - fracPart;
        tmp32no2 *= tmp16;
        tmp32no2 >>= 13;
        tmp32no2 = (1 << 14) - tmp32no2;
      } else {
        tmp16 = (int16_t)(constLinApprox - (1 << 14));
        tmp32no2 = (fracPart * tmp16) >> 13;
      }
      fracPart = (uint16_t)tmp32no2;
      gainTable[i] = wadd(wshl(1, intPart), shift_w32(fracPart, (int)intPart - 14));
    } else {
      gainTable[i] = 0;
    }
  }
  return 0;
}

// The sub-frame envelope: env[k] = max x^2 over sub-frame k (L = 8 or 16 samples); every lane gets all ten
template <int W>
AGC_HD inline void envelope(const int16_t* x, int L, int32_t* env, const Grp<W>& g, bool write) {
  for (int k = 0; k < 10; ++k) {
    int32_t m = 0;
    for (int i = g.lane; i < L; i += W) {
      const int32_t v = x[k * L + i] * x[k * L + i];
      m = v > m ? v : m;
    }
    m = g.max(m);
    if (write) env[k] = m;
  }
}

// ProcessDigital after its near-end VAD, up to the gains of the frame: w.gains[0..10], state.gain.
// Lane 0: decay, the capacitors, the gate; the limiter loop runs one sub-frame per lane.
template <int W>
AGC_HD inline void digital_gains(AspAgcState& s, AgcWork& w, int16_t logratio, const Grp<W>& g) {
  int32_t* gains = w.gains;
  const int32_t* env = w.env;
  if (g.is(0)) {
    if (s.vadFarend_counter > 10) logratio = (int16_t)((3 * logratio - s.vadFarend_logRatio) >> 2);
    int16_t decay;
    if (logratio > 1024)
      decay = -65;
    else if (logratio < 0)
      decay = 0;
    else
      decay = (int16_t)(((0 - logratio) * 65) >> 10);
    if (s.digitalAgc_agcMode != kAgcModeFixedDigital) {
      if (s.vadNearend_stdLongTerm < 4000)
        decay = 0;
      else if (s.vadNearend_stdLongTerm < 8096)
        decay = (int16_t)(((s.vadNearend_stdLongTerm - 4000) * decay) >> 12);
      if (s.lowLevelSignal != 0) decay = 0;
    }
    int32_t fast = s.digitalAgc_capacitorFast, slow = s.digitalAgc_capacitorSlow;
    int16_t zeros = 0, frac = 0;
    gains[0] = s.digitalAgc_gain;
    for (int k = 0; k < 10; k++) {
      fast = agc_scalediff32(-1000, fast, fast);
      if (env[k] > fast) fast = env[k];
      if (env[k] > slow)
        slow = agc_scalediff32(500, wsub(env[k], slow), slow);
      else
        slow = agc_scalediff32(decay, slow, slow);
      const int32_t cur_level = fast > slow ? fast : slow;
      zeros = norm_u32((uint32_t)cur_level);
      if (cur_level == 0) zeros = 31;
      const int32_t t = wshl(cur_level, zeros) & 0x7FFFFFFF;
      frac = (int16_t)(t >> 19);
      const int hi = zeros < 1 ? 0 : zeros - 1;   // zeros >= 1 for every level >= 0
      const int32_t d = wmul(wsub(s.digitalAgc_gainTable[hi], s.digitalAgc_gainTable[zeros]), frac);
      gains[k + 1] = wadd(s.digitalAgc_gainTable[zeros], d >> 12);
    }
    s.digitalAgc_capacitorFast = fast;
    s.digitalAgc_capacitorSlow = slow;
    // the gate
    zeros = (int16_t)((zeros << 9) - (frac >> 3));
    int16_t zeros_fast = norm_u32((uint32_t)fast);
    if (fast == 0) zeros_fast = 31;
    const int32_t t = wshl(fast, zeros_fast) & 0x7FFFFFFF;
    zeros_fast = (int16_t)(zeros_fast << 9);
    zeros_fast = (int16_t)(zeros_fast - (int16_t)(t >> 22));
    int16_t gate = (int16_t)(1000 + zeros_fast - zeros - s.vadNearend_stdShortTerm);
    if (gate < 0) {
      s.digitalAgc_gatePrevious = 0;
    } else {
      gate = (int16_t)((gate + s.digitalAgc_gatePrevious * 7) >> 3);
      s.digitalAgc_gatePrevious = gate;
    }
    if (gate > 0) {
      const int16_t gain_adj = gate < 2500 ? (int16_t)((2500 - gate) >> 5) : (int16_t)0;
      const int32_t g0 = s.digitalAgc_gainTable[0];
      for (int k = 0; k < 10; k++) {
        int32_t t2;
        if (wsub(gains[k + 1], g0) > 8388608) {
          t2 = wsub(gains[k + 1], g0) >> 8;
          t2 = wmul(t2, 178 + gain_adj);
        } else {
          t2 = wmul(wsub(gains[k + 1], g0), 178 + gain_adj);
          t2 >>= 8;
        }
        gains[k + 1] = wadd(g0, t2);
      }
    }
  }
  wsync();
  // the limiter: sub-frame k on lane k
  for (int k = g.lane; k < 10; k += W) {
    int32_t gk = gains[k + 1];
    int zeros = 10;
    if (gk > 47453132) zeros = 16 - norm_w32(gk);
    int32_t gain32 = wadd(gk >> zeros, 1);
    gain32 = wmul(gain32, gain32);
    const int32_t bound = shift_w32(32767, 2 * (1 - zeros + 10));
    const int32_t e = (env[k] >> 12) + 1;
    while (agc_mul32(e, gain32) > bound) {
      if (gk > 8388607)
        gk = (gk / 256) * 253;
      else
        gk = wmul(gk, 253) / 256;
      gain32 = wadd(gk >> zeros, 1);
      gain32 = wmul(gain32, gain32);
    }
    gains[k + 1] = gk;
  }
  wsync();
  if (g.is(0)) {
    for (int k = 1; k < 10; k++)
      if (gains[k] > gains[k + 1]) gains[k] = gains[k + 1];
    s.digitalAgc_gain = gains[10];
  }
  wsync();
}

// The gain ramp over the frame, every band: sample n of sub-frame k gets gains[k] * 16 + n * delta
template <int W>
AGC_HD inline void apply_gains(AgcWork& w, int nb, int L, const Grp<W>& g) {
  const int sh = L == 8 ? 1 : 0;   // 4 - L2
  for (int k = 0; k < 10; ++k) {
    const int32_t delta = wshl(wsub(w.gains[k + 1], w.gains[k]), sh);
    const int32_t base = wshl(w.gains[k], 4);
    for (int n = g.lane; n < L; n += W) {
      const int32_t gain32 = wadd(base, wmul(delta, n));
      for (int b = 0; b < nb; ++b) {
        int16_t* p = &w.x[b][k * L + n];
        const int32_t x = *p;
        if (k == 0) {
          const int32_t out_tmp = wmul(x, wadd(gain32, 127) >> 7) >> 16;
          if (out_tmp > 4095) {
            *p = 32767;
            continue;
          }
          if (out_tmp < -4096) {
            *p = -32768;
            continue;
          }
        }
        *p = (int16_t)(wmul(x, gain32 >> 4) >> 16);
      }
    }
  }
}

// ------------------------------------------------------------------ analog_agc.c
AGC_HD inline void update_agc_thresholds(AspAgcState& s) {
  int16_t tmp16 = (int16_t)(5 * s.compressionGaindB + 5);
  tmp16 = div_w32w16_res16(tmp16, 11);
  s.analogTarget = (int16_t)(4 + tmp16);
  if (s.analogTarget < 4) s.analogTarget = 4;
  if (s.agcMode == kAgcModeFixedDigital) s.analogTarget = s.compressionGaindB;
  s.targetIdx = 20;
  s.analogTargetLevel = 10 * kTargetLevelTable[s.targetIdx];
  s.startUpperLimit = 10 * kTargetLevelTable[s.targetIdx - 1];
  s.startLowerLimit = 10 * kTargetLevelTable[s.targetIdx + 1];
  s.upperPrimaryLimit = 10 * kTargetLevelTable[s.targetIdx - 2];
  s.lowerPrimaryLimit = 10 * kTargetLevelTable[s.targetIdx + 2];
  s.upperSecondaryLimit = 10 * kTargetLevelTable[s.targetIdx - 5];
  s.lowerSecondaryLimit = 10 * kTargetLevelTable[s.targetIdx + 5];
  s.upperLimit = s.startUpperLimit;
  s.lowerLimit = s.startLowerLimit;
}

// WebRtcAgc_set_config (the handle is not NULL)
AGC_HD inline int set_config_core(AspAgcState& s, int16_t targetLevelDbfs, int16_t compressionGaindB, uint8_t limiterEnable) {
  if (s.initFlag != 42) {
    s.lastError = (int16_t)AGC_UNINITIALIZED_ERROR;
    return -1;
  }
  if (limiterEnable != kAgcFalse && limiterEnable != kAgcTrue) {
    s.lastError = (int16_t)AGC_BAD_PARAMETER_ERROR;
    return -1;
  }
  s.limiterEnable = limiterEnable;
  s.compressionGaindB = compressionGaindB;
  if (targetLevelDbfs < 0 || targetLevelDbfs > 31) {
    s.lastError = (int16_t)AGC_BAD_PARAMETER_ERROR;
    return -1;
  }
  s.targetLevelDbfs = targetLevelDbfs;
  if (s.agcMode == kAgcModeFixedDigital) s.compressionGaindB = (int16_t)(s.compressionGaindB + targetLevelDbfs);
  update_agc_thresholds(s);
  if (calculate_gain_table(s.digitalAgc_gainTable, s.compressionGaindB, s.targetLevelDbfs, s.limiterEnable,
                           s.analogTarget) == -1)
    return -1;
  s.usedConfig_compressionGaindB = compressionGaindB;
  s.usedConfig_limiterEnable = limiterEnable;
  s.usedConfig_targetLevelDbfs = targetLevelDbfs;
  return 0;
}

// WebRtcAgc_Init; fs and the mode were checked by the caller (asp_agc.h)
AGC_HD inline int init_core(AspAgcState& s, int32_t minLevel, int32_t maxLevel, int16_t agcMode, uint32_t fs) {
  s.digitalAgc_capacitorSlow = agcMode == kAgcModeFixedDigital ? 0 : 134217728;
  s.digitalAgc_capacitorFast = 0;
  s.digitalAgc_gain = 65536;
  s.digitalAgc_gatePrevious = 0;
  s.digitalAgc_agcMode = agcMode;
  init_vad(AGC_VAD(s, vadNearend));
  init_vad(AGC_VAD(s, vadFarend));
  s.envSum = 0;
  s.agcMode = agcMode;
  s.fs = fs;
  init_vad(AGC_VAD(s, vadMic));
  s.scale = 0;
  if (s.agcMode == kAgcModeAdaptiveDigital) {
    minLevel = 0;
    maxLevel = 255;
  }
  const int32_t max_add = wsub(maxLevel, minLevel) / 4;
  s.minLevel = minLevel;
  s.maxAnalog = maxLevel;
  s.maxLevel = wadd(maxLevel, max_add);
  s.maxInit = s.maxLevel;
  s.zeroCtrlMax = s.maxAnalog;
  s.lastInMicLevel = 0;
  s.micVol = s.maxAnalog;
  if (s.agcMode == kAgcModeAdaptiveDigital) s.micVol = 127;
  s.micRef = s.micVol;
  s.micGainIdx = 127;
  s.minOutput = wadd(s.minLevel, wmul(wsub(s.maxLevel, s.minLevel), 10) >> 8);
  s.msTooLow = 0;
  s.msTooHigh = 0;
  s.changeToSlowMode = 0;
  s.firstCall = 0;
  s.msZero = 0;
  s.muteGuardMs = 0;
  s.gainTableIdx = 0;
  s.msecSpeechInnerChange = 520;
  s.msecSpeechOuterChange = 340;
  s.activeSpeech = 0;
  s.Rxx16_LPw32Max = 0;
  s.vadThreshold = 400;
  s.inActive = 0;
  for (int i = 0; i < 10; i++) s.Rxx16_vectorw32[i] = 1000;
  s.Rxx160w32 = 125 * 10;
  s.Rxx16pos = 0;
  s.Rxx16_LPw32 = 16284;
  for (int i = 0; i < 5; i++) s.Rxx16w32_array[0][i] = 0;
  for (int i = 0; i < 10; i++) {
    s.env[0][i] = 0;
    s.env[1][i] = 0;
  }
  s.inQueue = 0;
  for (int i = 0; i < 8; i++) s.filterState[i] = 0;
  s.initFlag = 42;
  s.defaultConfig_limiterEnable = kAgcTrue;
  s.defaultConfig_targetLevelDbfs = 3;
  s.defaultConfig_compressionGaindB = 9;
  if (set_config_core(s, 3, 9, kAgcTrue) == -1) {
    s.lastError = (int16_t)AGC_UNSPECIFIED_ERROR;
    return -1;
  }
  s.Rxx160_LPw32 = s.analogTargetLevel;
  s.lowLevelSignal = 0;
  if (minLevel >= maxLevel || (maxLevel & 0xFC000000)) return -1;
  return 0;
}

AGC_HD inline int tab128(int32_t i) { return i < 0 ? 0 : i > 127 ? 127 : i; }
AGC_HD inline uint16_t virtual_mic_gain(int32_t gainIdx, int after_clip) {
  // before the loop: gainIdx > 127 reads the gain table at gainIdx - 128; after a clip: gainIdx >= 127 reads it at gainIdx - 127
  if (after_clip ? gainIdx >= 127 : gainIdx > 127) return kGainTableVirtualMic[tab128(gainIdx - (after_clip ? 127 : 128))];
  return kSuppressionTableVirtualMic[tab128(127 - gainIdx)];
}

// WebRtcAgc_VirtualMic up to its call of AddMic: the low-level decision, then the emulated microphone gain on
// w.x.  Returns micLevelOut on every lane.
template <int W>
AGC_HD inline int32_t virtual_mic_core(AspAgcState& s, AgcWork& w, int nb, int n, int32_t micLevelIn, const Grp<W>& g) {
  const int16_t* x = w.x[0];
  const uint32_t limit = s.fs != 8000 ? 11000u : 5500u;
  // frame energy up to the limit, and the zero crossings
  int32_t part = 0, zc = 0;
  for (int i = g.lane; i < n; i += W) {
    const uint32_t e = (uint32_t)(x[i] * x[i]);
    part += (int32_t)(e < limit ? e : limit);
    if (i > 0) zc += ((x[i] ^ x[i - 1]) < 0);
  }
  const uint32_t total = (uint32_t)g.sum(part);
  zc = g.sum(zc);
  if (g.is(0)) {
    uint32_t frameNrg = total;
    if (total >= limit) {   // the first prefix sum at or over the limit is what the reference holds
      frameNrg = (uint32_t)(x[0] * x[0]);
      for (int i = 1; i < n && frameNrg < limit; ++i) frameNrg += (uint32_t)(x[i] * x[i]);
    }
    const int16_t numZeroCrossing = (int16_t)zc;
    if (frameNrg < 500 || numZeroCrossing <= 5)
      s.lowLevelSignal = 1;
    else if (numZeroCrossing <= 15)
      s.lowLevelSignal = 0;
    else if (frameNrg <= limit)
      s.lowLevelSignal = 1;
    else if (numZeroCrossing >= 20)
      s.lowLevelSignal = 1;
    else
      s.lowLevelSignal = 0;
    int32_t gainIdx = s.micVol;
    if (s.micVol > s.maxAnalog) gainIdx = s.maxAnalog;
    if (micLevelIn != s.micRef) {
      s.micRef = micLevelIn;
      s.micVol = 127;
      s.micGainIdx = 127;
      gainIdx = 127;
    }
    w.sc[0] = gainIdx;
  }
  wsync();
  int32_t gainIdx = w.sc[0];
  uint16_t gain = virtual_mic_gain(gainIdx, 0);
  // does any low-band sample clip at the starting gain?
  int32_t clip = 0;
  for (int i = g.lane; i < n; i += W) {
    const int32_t v = (x[i] * gain) >> 10;
    clip |= (v > 32767 || v < -32768);
  }
  clip = g.max(clip);
  if (!clip) {
    for (int b = 0; b < nb; ++b)
      for (int i = g.lane; i < n; i += W) w.x[b][i] = sat16((w.x[b][i] * gain) >> 10);
  } else if (g.is(0)) {   // the gain steps down at every clipped sample: in order
    for (int i = 0; i < n; ++i) {
      int32_t v = (w.x[0][i] * gain) >> 10;
      if (v > 32767) {
        v = 32767;
        gainIdx--;
        gain = virtual_mic_gain(gainIdx, 1);
      }
      if (v < -32768) {
        v = -32768;
        gainIdx--;
        gain = virtual_mic_gain(gainIdx, 1);
      }
      w.x[0][i] = (int16_t)v;
      for (int b = 1; b < nb; ++b) w.x[b][i] = sat16((w.x[b][i] * gain) >> 10);
    }
    w.sc[0] = gainIdx;
  }
  wsync();
  gainIdx = w.sc[0];
  if (g.is(0)) s.micGainIdx = gainIdx;
  wsync();
  return gainIdx;
}

// WebRtcAgc_AddMic before its VAD and its decimator (mic_serial below): the slowly varying digital gain and
// the envelope, into the half of the queue that inQueue selects.
template <int W>
AGC_HD inline void add_mic_gain_env(AspAgcState& s, AgcWork& w, int nb, int n, const Grp<W>& g) {
  if (g.is(0)) {
    int32_t gain = 0;
    if (s.micVol > s.maxAnalog) {
      int16_t tmp16 = (int16_t)(s.micVol - s.maxAnalog);
      const int32_t tmp32 = 31 * tmp16;
      tmp16 = (int16_t)(s.maxLevel - s.maxAnalog);
      const uint16_t targetGainIdx = (uint16_t)(tmp16 != 0 ? tmp32 / tmp16 : 0);
      if (s.gainTableIdx < targetGainIdx)
        s.gainTableIdx++;
      else if (s.gainTableIdx > targetGainIdx)
        s.gainTableIdx--;
      gain = kGainTableAnalog[s.gainTableIdx > 31 ? 31 : s.gainTableIdx];
    } else {
      s.gainTableIdx = 0;
    }
    w.sc[1] = gain;
  }
  wsync();
  const int32_t gain = w.sc[1];
  if (gain) {
    for (int b = 0; b < nb; ++b)
      for (int i = g.lane; i < n; i += W) w.x[b][i] = sat16((w.x[b][i] * gain) >> 12);
    wsync();
  }
  envelope(w.x[0], n / 10, s.env[s.inQueue > 0 ? 1 : 0], g, g.is(0));
}

// AddMic's five block energies, from the decimated low band (fs == 16000) or the first 80 samples
template <int W>
AGC_HD inline void add_mic_energy(AspAgcState& s, AgcWork& w, const Grp<W>& g) {
  const int16_t* src = s.fs == 16000 ? w.ds : w.x[0];
  int32_t* dst = s.Rxx16w32_array[s.inQueue > 0 ? 1 : 0];
  for (int i = 0; i < 5; ++i) {
    int32_t p = 0;
    for (int k = g.lane; k < 16; k += W) p = wadd(p, (src[i * 16 + k] * src[i * 16 + k]) >> 4);
    p = g.sum(p);
    if (g.is(0)) dst[i] = p;
  }
  wsync();
  if (g.is(0)) s.inQueue = s.inQueue == 0 ? 1 : 2;
}

AGC_HD inline int16_t exp_curve(int16_t volume) {
  if (volume > 5243) {
    if (volume > 7864) return volume > 12124 ? 7 : 6;
    return volume > 6554 ? 5 : 4;
  }
  if (volume > 2621) return volume > 3932 ? 3 : 2;
  return volume > 1311 ? 1 : 0;
}

// level = ((factor * (level - minLevel)) >> shift) + minLevel in unsigned arithmetic
AGC_HD inline int32_t scale_level(uint32_t factor, int32_t level, int32_t minLevel, int shift) {
  return (int32_t)(((factor * (uint32_t)wsub(level, minLevel)) >> shift) + (uint32_t)minLevel);
}

// WebRtcAgc_ProcessAnalog (one lane)
AGC_HD inline int32_t process_analog(AspAgcState& s, int32_t inMicLevel, int32_t* outMicLevel, int16_t vadLogRatio,
                                     int16_t echo, uint8_t* saturationWarning) {
  int32_t inMicLevelTmp = inMicLevel;   // scale is 0
  if (inMicLevelTmp > s.maxAnalog) return -1;
  if (inMicLevelTmp < s.minLevel) return -1;
  if (s.firstCall == 0) {
    s.firstCall = 1;
    const int32_t tmpVol = wadd(s.minLevel, wmul(wsub(s.maxLevel, s.minLevel), 51) >> 9);
    if (inMicLevelTmp < tmpVol && s.agcMode == kAgcModeAdaptiveAnalog) inMicLevelTmp = tmpVol;
    s.micVol = inMicLevelTmp;
  }
  if (inMicLevelTmp == s.maxAnalog && s.micVol > s.maxAnalog) inMicLevelTmp = s.micVol;
  if (inMicLevelTmp != s.micVol && inMicLevelTmp < s.minOutput) {
    inMicLevelTmp = wadd(s.minLevel, wmul(wsub(s.maxLevel, s.minLevel), 51) >> 9);
    s.micVol = inMicLevelTmp;
  }
  if (inMicLevelTmp != s.micVol) {
    if (inMicLevel == s.lastInMicLevel)
      inMicLevelTmp = s.micVol;
    else
      s.micVol = inMicLevelTmp;
  }
  if (inMicLevelTmp > s.maxLevel) s.maxLevel = inMicLevelTmp;
  s.lastInMicLevel = inMicLevel;
  const int32_t lastMicVol = s.micVol;

  // SaturationCtrl on the older envelope
  uint8_t saturated = 0;
  for (int i = 0; i < 10; i++) {
    const int16_t t = (int16_t)(s.env[0][i] >> 20);
    if (t > 875) s.envSum = (int16_t)(s.envSum + t);
  }
  if (s.envSum > 25000) {
    saturated = 1;
    s.envSum = 0;
  }
  s.envSum = (int16_t)((s.envSum * 32440) >> 15);
  if (saturated == 1) {
    s.Rxx160_LPw32 = (s.Rxx160_LPw32 / 8) * 7;
    s.zeroCtrlMax = s.micVol;
    s.micVol = scale_level(29591, inMicLevelTmp, s.minLevel, 15);
    if (s.micVol > lastMicVol - 2) s.micVol = lastMicVol - 2;
    inMicLevelTmp = s.micVol;
    if (s.micVol < s.minOutput) *saturationWarning = 1;
    s.msTooHigh = -100;
    s.activeSpeech = 0;
    s.Rxx16_LPw32Max = 0;
    s.msecSpeechInnerChange = 520;
    s.msecSpeechOuterChange = 340;
    s.changeToSlowMode = 0;
    s.muteGuardMs = 0;
    s.upperLimit = s.startUpperLimit;
    s.lowerLimit = s.startLowerLimit;
  }

  // ZeroCtrl
  {
    int32_t sum = 0;
    for (int i = 0; i < 10; i++) sum = wadd(sum, s.env[0][i]);
    if (sum < 500)
      s.msZero = (int16_t)(s.msZero + 10);
    else
      s.msZero = 0;
    if (s.muteGuardMs > 0) s.muteGuardMs = (int16_t)(s.muteGuardMs - 10);
    if (s.msZero > 500) {
      s.msZero = 0;
      const int32_t midVal = wadd(wadd(s.maxAnalog, s.minLevel), 1) / 2;
      if (inMicLevelTmp < midVal) {
        inMicLevelTmp = wmul(1126, inMicLevelTmp) >> 10;
        inMicLevelTmp = inMicLevelTmp < s.zeroCtrlMax ? inMicLevelTmp : s.zeroCtrlMax;
        s.micVol = inMicLevelTmp;
      }
      s.activeSpeech = 0;
      s.Rxx16_LPw32Max = 0;
      s.muteGuardMs = 8000;
    }
  }

  // SpeakerInactiveCtrl
  if (s.vadMic_stdLongTerm < 2500) {
    s.vadThreshold = 1500;
  } else {
    int16_t vadThresh = 400;
    if (s.vadMic_stdLongTerm < 4500) vadThresh = (int16_t)(vadThresh + (4500 - s.vadMic_stdLongTerm) / 2);
    s.vadThreshold = (int16_t)((vadThresh + 31 * s.vadThreshold) >> 5);
  }

  for (int i = 0; i < 5; i++) {
    const int32_t Rxx16w32 = s.Rxx16w32_array[0][i];
    const int pos = s.Rxx16pos < 0 ? 0 : s.Rxx16pos > 9 ? 9 : s.Rxx16pos;
    int32_t tmp32 = wsub(Rxx16w32, s.Rxx16_vectorw32[pos]) >> 3;
    s.Rxx160w32 = wadd(s.Rxx160w32, tmp32);
    s.Rxx16_vectorw32[pos] = Rxx16w32;
    s.Rxx16pos = (int16_t)(pos + 1);
    if (s.Rxx16pos == 10) s.Rxx16pos = 0;
    tmp32 = wsub(Rxx16w32, s.Rxx16_LPw32) >> 6;
    s.Rxx16_LPw32 = wadd(s.Rxx16_LPw32, tmp32);

    if (vadLogRatio > s.vadThreshold) {
      if (s.activeSpeech < 250) {
        s.activeSpeech = (int16_t)(s.activeSpeech + 2);
        if (s.Rxx16_LPw32 > s.Rxx16_LPw32Max) s.Rxx16_LPw32Max = s.Rxx16_LPw32;
      } else if (s.activeSpeech == 250) {
        s.activeSpeech = (int16_t)(s.activeSpeech + 2);
        s.Rxx160_LPw32 = wmul(s.Rxx16_LPw32Max >> 3, 10);
      }
      tmp32 = wsub(s.Rxx160w32, s.Rxx160_LPw32) >> 10;
      s.Rxx160_LPw32 = wadd(s.Rxx160_LPw32, tmp32);

      if (s.Rxx160_LPw32 > s.upperSecondaryLimit || s.Rxx160_LPw32 > s.upperLimit) {
        const bool outer = s.Rxx160_LPw32 > s.upperSecondaryLimit;
        s.msTooHigh = (int16_t)(s.msTooHigh + 2);
        s.msTooLow = 0;
        s.changeToSlowMode = 0;
        if (s.msTooHigh > (outer ? s.msecSpeechOuterChange : s.msecSpeechInnerChange)) {
          s.msTooHigh = 0;
          // times 53 / 64: the outer branch shifts, the inner one divides
          s.Rxx160_LPw32 = outer ? wmul(s.Rxx160_LPw32 >> 6, 53) : (s.Rxx160_LPw32 / 64) * 53;
          s.maxLevel = wadd(wmul(15, s.maxLevel), s.micVol) / 16;
          s.maxLevel = s.maxLevel > s.maxAnalog ? s.maxLevel : s.maxAnalog;
          s.zeroCtrlMax = s.micVol;
          s.micVol = scale_level(outer ? 31130 : 31621, inMicLevelTmp, s.minLevel, 15);
          if (s.micVol > lastMicVol - 1) s.micVol = lastMicVol - 1;
          inMicLevelTmp = s.micVol;
          if (outer) {
            s.activeSpeech = 0;
            s.Rxx16_LPw32Max = 0;
          }
        }
      } else if (s.Rxx160_LPw32 < s.lowerSecondaryLimit || s.Rxx160_LPw32 < s.lowerLimit) {
        const bool outer = s.Rxx160_LPw32 < s.lowerSecondaryLimit;
        s.msTooHigh = 0;
        s.changeToSlowMode = 0;
        s.msTooLow = (int16_t)(s.msTooLow + 2);
        if (s.msTooLow > (outer ? s.msecSpeechOuterChange : s.msecSpeechInnerChange)) {
          int16_t volNormFIX = 16384;
          s.msTooLow = 0;
          const int32_t tmp = wshl(wsub(inMicLevelTmp, s.minLevel), 14);
          if (s.maxInit != s.minLevel) volNormFIX = (int16_t)(tmp / wsub(s.maxInit, s.minLevel));
          const int16_t index = exp_curve(volNormFIX);
          const int16_t weightFIX = outer ? (int16_t)(kOffset1[index] - (int16_t)((kSlope1[index] * volNormFIX) >> 13))
                                          : (int16_t)(kOffset2[index] - (int16_t)((kSlope2[index] * volNormFIX) >> 13));
          s.Rxx160_LPw32 = (s.Rxx160_LPw32 / 64) * 67;
          s.micVol = scale_level((uint32_t)(int32_t)weightFIX, inMicLevelTmp, s.minLevel, 14);
          const int32_t step = outer ? 2 : 1;
          if (s.micVol < lastMicVol + step) s.micVol = lastMicVol + step;
          inMicLevelTmp = s.micVol;
        }
      } else {
        if (s.changeToSlowMode > 4000) {
          s.msecSpeechInnerChange = 1000;
          s.msecSpeechOuterChange = 500;
          s.upperLimit = s.upperPrimaryLimit;
          s.lowerLimit = s.lowerPrimaryLimit;
        } else {
          s.changeToSlowMode = (int16_t)(s.changeToSlowMode + 2);
        }
        s.msTooLow = 0;
        s.msTooHigh = 0;
        s.micVol = inMicLevelTmp;
      }
    }
  }

  if (echo == 1 || (s.muteGuardMs > 0 && s.muteGuardMs < 8000)) {
    if (s.micVol > lastMicVol) s.micVol = lastMicVol;
  }
  if (s.micVol > s.maxLevel)
    s.micVol = s.maxLevel;
  else if (s.micVol < s.minOutput)
    s.micVol = s.minOutput;
  *outMicLevel = s.micVol < s.maxAnalog ? s.micVol : s.maxAnalog;
  return 0;
}

// ------------------------------------------------------------------ one frame
// ops of a frame; kOpByMode picks AddMic / VirtualMic / neither from the stream's mode (the fused call)
enum { kOpFar = 1, kOpAddMic = 2, kOpVirtualMic = 4, kOpProcess = 8, kOpByMode = 16 };

struct FrameIo {
  int32_t level_in;    // micLevelIn of VirtualMic, inMicLevel of Process
  int16_t echo;
  int32_t vm_level;    // out: VirtualMic's micLevelOut
  int32_t level_out;   // out: Process's outMicLevel
  uint8_t saturation;  // out
  int32_t rc;          // out: the reference's return value of the last operation run
};

// The audio of the frame is staged in w.x (bands) and w.far; the result is left in w.x.  The scalar outputs
// of io are valid on lane 0.
template <int W>
AGC_HD inline void frame_core(AspAgcState& s, AgcWork& w, int ops, int nb, int n, FrameIo& io, const Grp<W>& g) {
  if (ops & kOpByMode) {
    ops &= ~(kOpAddMic | kOpVirtualMic);
    if (s.agcMode == kAgcModeAdaptiveAnalog) ops |= kOpAddMic;
    if (s.agcMode == kAgcModeAdaptiveDigital) ops |= kOpVirtualMic;
  }
  const bool mic = (ops & (kOpAddMic | kOpVirtualMic)) != 0;
  io.rc = 0;
  io.vm_level = io.level_in;
  int32_t process_level = io.level_in;
  if (ops & kOpVirtualMic) {
    io.vm_level = virtual_mic_core(s, w, nb, n, io.level_in, g);
    process_level = io.vm_level;
  }
  if (mic) add_mic_gain_env(s, w, nb, n, g);
  wsync();
  // the three AgcVad chains in one pass: role r = 0 near end, 1 far end, 2 microphone sits on lane r of the
  // group (the CPU's single lane takes the roles in turn); one copy of the loop, state and input picked by r
  for (int r = g.lane; r < 3; r += W) {
    const bool on = r == 0 ? (ops & kOpProcess) != 0 : r == 1 ? (ops & kOpFar) != 0 : mic;
    const VadRef v = r == 0 ? AGC_VAD(s, vadNearend) : r == 1 ? AGC_VAD(s, vadFarend) : AGC_VAD(s, vadMic);
    const int16_t* in = r == 1 ? w.far : w.x[0];
    if (on) {
      const int16_t lr = process_vad(v, in, n);
      if (r == 0) w.sc[2] = lr;
    }
  }
  // then AddMic's by-2 decimator, a pass of its own on lane 3
  if (mic && s.fs == 16000 && g.is(3)) {
    Ds2 d = ds2_load(s.filterState);
    for (int i = 0; i < 80; ++i) w.ds[i] = ds2_step(d, w.x[0][2 * i], w.x[0][2 * i + 1]);
    ds2_store(s.filterState, d);
  }
  wsync();
  if (mic) add_mic_energy(s, w, g);
  if (!(ops & kOpProcess)) return;
  wsync();
  const int L = n / 10;
  envelope(w.x[0], L, w.env, g, g.is(0));
  wsync();
  digital_gains(s, w, (int16_t)w.sc[2], g);
  apply_gains(w, nb, L, g);
  wsync();
  if (g.is(0)) {
    io.saturation = 0;
    io.level_out = process_level;
    if (s.agcMode < kAgcModeFixedDigital && (s.lowLevelSignal == 0 || s.agcMode != kAgcModeAdaptiveDigital))
      io.rc = process_analog(s, process_level, &io.level_out, s.vadMic_logRatio, io.echo, &io.saturation);
    if (io.rc == 0) {
      if (s.inQueue > 1) {
        for (int i = 0; i < 10; ++i) s.env[0][i] = s.env[1][i];
        for (int i = 0; i < 5; ++i) s.Rxx16w32_array[0][i] = s.Rxx16w32_array[1][i];
      }
      if (s.inQueue > 0) s.inQueue--;
    }
  }
  wsync();
}

}  // namespace aspagc
#endif  // ASP_AGC_CORE_H_
