// aecm_core.h -- one stream of the mobile echo canceller, restated with the reference's integer
// semantics (echo_control_mobile.c, aecm_core.c, aecm_core_c.c, delay_estimator*.c, ring_buffer.c and
// the spl helpers it calls).  Every function works on one AspAecmState and one AecmWork in global memory:
// the kernel (aecm_kernels.hip) runs it with one lane per stream; nothing here keeps an array in private
// memory, so the kernel needs no scratch.  Wrapping int32 arithmetic is written as uint32 arithmetic
// where the reference relies on the compiler's two's-complement wrap.
#ifndef ASP_AECM_CORE_H_
#define ASP_AECM_CORE_H_

#include "aecm_layout.h"

namespace aspaecm {

// ------------------------------------------------------------------ spl helpers (spl_inl.h, *.c)
AECM_HD inline int norm_u32(uint32_t a) {
  if (a == 0) return 0;
  return __builtin_clz(a);
}
AECM_HD inline int norm_w32(int32_t a) {
  if (a == 0) return 0;
  uint32_t u = (uint32_t)(a < 0 ? ~a : a);
  return u == 0 ? 31 : __builtin_clz(u) - 1;  // u < 2^31
}
AECM_HD inline int norm_w16(int a16) {
  int32_t a = (int16_t)a16;
  if (a == 0) return 0;
  uint32_t u = (uint32_t)(a < 0 ? ~a : a);  // < 2^15
  return u == 0 ? 15 : __builtin_clz(u) - 17;
}
AECM_HD inline int32_t add_sat_w32(int32_t a, int32_t b) {
  int32_t s = (int32_t)((uint32_t)a + (uint32_t)b);
  if (a < 0) {
    if (b < 0 && s >= 0) s = (int32_t)0x80000000;
  } else if (b > 0 && s < 0) {
    s = 0x7FFFFFFF;
  }
  return s;
}
AECM_HD inline int16_t sat_w16(int32_t v) { return (int16_t)(v > 32767 ? 32767 : v < -32768 ? -32768 : v); }
AECM_HD inline int32_t div_w32w16(int32_t num, int den16) {
  int16_t den = (int16_t)den16;
  return den != 0 ? num / den : 0x7FFFFFFF;
}
AECM_HD inline uint32_t div_u32u16(uint32_t num, uint16_t den) { return den != 0 ? num / den : 0xFFFFFFFFu; }
AECM_HD inline int32_t sqrt_floor(int32_t value) {
  int32_t root = 0;
  for (int n = 15; n >= 0; --n) {
    int32_t t = root + (1 << n);
    if (value >= (int32_t)((uint32_t)t << n)) {
      value -= (int32_t)((uint32_t)t << n);
      root |= 2 << n;
    }
  }
  return root >> 1;
}
AECM_HD inline int max_abs_w16(const int16_t* v, int n) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    int a = v[i] < 0 ? -v[i] : v[i];
    if (a > m) m = a;
  }
  return m > 32767 ? 32767 : m;
}
// WEBRTC_SPL_SHIFT_W32 on signed and unsigned values (left shifts as unsigned: defined wrap)
AECM_HD inline int32_t shift_w32(int32_t x, int c) { return c >= 0 ? (int32_t)((uint32_t)x << c) : x >> -c; }
AECM_HD inline uint32_t shift_u32(uint32_t x, int c) { return c >= 0 ? x << c : x >> -c; }
AECM_HD inline int16_t abs_w16(int16_t a) { return (int16_t)(a >= 0 ? a : -a); }
AECM_HD inline int32_t mul16(int a, int b) { return (int32_t)(int16_t)a * (int32_t)(int16_t)b; }

// ------------------------------------------------------------------ RingBuffer (ring_buffer.c)
AECM_HD inline int ring_avail_read(const AspAecmRing& r, int count) {
  return r.rw_wrap == 0 ? r.write_pos - r.read_pos : count - r.read_pos + r.write_pos;
}
AECM_HD inline int ring_move(AspAecmRing& r, int count, int n) {
  const int free_el = count - ring_avail_read(r, count);
  const int readable = ring_avail_read(r, count);
  int pos = r.read_pos;
  if (n > readable) n = readable;
  if (n < -free_el) n = -free_el;
  pos += n;
  if (pos > count) {
    pos -= count;
    r.rw_wrap = 0;
  }
  if (pos < 0) {
    pos += count;
    r.rw_wrap = 1;
  }
  r.read_pos = pos;
  return n;
}
AECM_HD inline void ring_write(AspAecmRing& r, int16_t* data, int count, const int16_t* src, int n) {
  const int free_el = count - ring_avail_read(r, count);
  const int w = free_el < n ? free_el : n;
  int left = w;
  const int margin = count - r.write_pos;
  if (w > margin) {
    for (int i = 0; i < margin; ++i) data[r.write_pos + i] = src[i];
    r.write_pos = 0;
    left -= margin;
    r.rw_wrap = 1;
  }
  for (int i = 0; i < left; ++i) data[r.write_pos + i] = src[w - left + i];
  r.write_pos += left;
}
// reads up to n elements into dst (the elements the reference's pointer / copy would show); returns the count
AECM_HD inline int ring_read(AspAecmRing& r, const int16_t* data, int count, int16_t* dst, int n) {
  const int readable = ring_avail_read(r, count);
  const int rd = readable < n ? readable : n;
  const int margin = count - r.read_pos;
  if (rd > margin) {
    for (int i = 0; i < margin; ++i) dst[i] = data[r.read_pos + i];
    for (int i = margin; i < rd; ++i) dst[i] = data[i - margin];
  } else {
    for (int i = 0; i < rd; ++i) dst[i] = data[r.read_pos + i];
  }
  ring_move(r, count, rd);
  return rd;
}
AECM_HD inline void ring_init(AspAecmRing& r, int16_t* data, int count) {
  r.read_pos = 0;
  r.write_pos = 0;
  r.rw_wrap = 0;
  for (int i = 0; i < count; ++i) data[i] = 0;
}

// ------------------------------------------------------------------ 128-point fixed-point FFT (order 7)
AECM_HD inline int bitrev7(int i) {
  int r = 0;
  for (int b = 0; b < 7; ++b) r |= ((i >> b) & 1) << (6 - b);
  return r;
}
// WebRtcSpl_ComplexBitReverse, stages 7: the swaps of index_7 are the pairs (i, rev7(i)), i < rev7(i)
AECM_HD inline void bit_reverse(int16_t* c) {
  for (int i = 1; i < 128; ++i) {
    const int r = bitrev7(i);
    if (i < r) {
      int16_t a = c[2 * i], b = c[2 * i + 1];
      c[2 * i] = c[2 * r];
      c[2 * i + 1] = c[2 * r + 1];
      c[2 * r] = a;
      c[2 * r + 1] = b;
    }
  }
}
// WebRtcSpl_ComplexFFT, mode 1
AECM_HD inline void complex_fft(int16_t* fr, const int16_t* sin1024) {
  int k = 9;
  for (int l = 1; l < 128; l <<= 1, --k) {
    const int istep = l << 1;
    for (int m = 0; m < l; ++m) {
      const int jj = m << k;
      const int wr = sin1024[jj + 256], wi = (int16_t)(-sin1024[jj]);
      for (int i = m; i < 128; i += istep) {
        const int j = i + l;
        int32_t tr = (wr * fr[2 * j] - wi * fr[2 * j + 1] + 1) >> 1;
        int32_t ti = (wr * fr[2 * j + 1] + wi * fr[2 * j] + 1) >> 1;
        const int32_t qr = (int32_t)fr[2 * i] << 14, qi = (int32_t)fr[2 * i + 1] << 14;
        fr[2 * j] = (int16_t)((qr - tr + 16384) >> 15);
        fr[2 * j + 1] = (int16_t)((qi - ti + 16384) >> 15);
        fr[2 * i] = (int16_t)((qr + tr + 16384) >> 15);
        fr[2 * i + 1] = (int16_t)((qi + ti + 16384) >> 15);
      }
    }
  }
}
// WebRtcSpl_ComplexIFFT, mode 1: a shift per stage from the data's max-abs; returns the total scale
AECM_HD inline int complex_ifft(int16_t* fr, const int16_t* sin1024) {
  int scale = 0, k = 9;
  for (int l = 1; l < 128; l <<= 1, --k) {
    int shift = 0;
    int32_t round2 = 8192;
    const int32_t mx = max_abs_w16(fr, 256);
    if (mx > 13573) {
      ++shift;
      ++scale;
      round2 <<= 1;
    }
    if (mx > 27146) {
      ++shift;
      ++scale;
      round2 <<= 1;
    }
    const int istep = l << 1;
    for (int m = 0; m < l; ++m) {
      const int jj = m << k;
      const int wr = sin1024[jj + 256], wi = sin1024[jj];
      for (int i = m; i < 128; i += istep) {
        const int j = i + l;
        int32_t tr = (wr * fr[2 * j] - wi * fr[2 * j + 1] + 1) >> 1;
        int32_t ti = (wr * fr[2 * j + 1] + wi * fr[2 * j] + 1) >> 1;
        const int32_t qr = (int32_t)fr[2 * i] << 14, qi = (int32_t)fr[2 * i + 1] << 14;
        fr[2 * j] = (int16_t)((qr - tr + round2) >> (shift + 14));
        fr[2 * j + 1] = (int16_t)((qi - ti + round2) >> (shift + 14));
        fr[2 * i] = (int16_t)((qr + tr + round2) >> (shift + 14));
        fr[2 * i + 1] = (int16_t)((qi + ti + round2) >> (shift + 14));
      }
    }
  }
  return scale;
}

// ------------------------------------------------------------------ fixed-point delay estimator
AECM_HD inline void mean_estimator_fix(int32_t nv, int factor, int32_t* mean) {
  int32_t diff = (int32_t)((uint32_t)nv - (uint32_t)*mean);
  diff = diff < 0 ? -((-diff) >> factor) : diff >> factor;
  *mean = (int32_t)((uint32_t)*mean + (uint32_t)diff);
}
// BinarySpectrumFix, bands 12..43
AECM_HD inline uint32_t binary_spectrum_fix(const uint16_t* sp, int32_t* thr, int q, int32_t* initialized) {
  uint32_t out = 0;
  if (!*initialized) {
    for (int i = 12; i <= 43; ++i)
      if (sp[i] > 0) {
        thr[i] = (int32_t)((uint32_t)sp[i] << (15 - q)) >> 1;
        *initialized = 1;
      }
  }
  for (int i = 12; i <= 43; ++i) {
    const int32_t s15 = (int32_t)((uint32_t)sp[i] << (15 - q));
    mean_estimator_fix(s15, 6, &thr[i]);
    if (s15 > thr[i]) out |= 1u << (i - 12);
  }
  return out;
}
AECM_HD inline void add_far_spectrum(AspAecmState& s, const uint16_t* far, int far_q) {
  const uint32_t bs = binary_spectrum_fix(far, s.mean_far_spectrum, far_q, &s.far_spectrum_initialized);
  for (int i = kMaxDelay - 1; i > 0; --i) {
    s.binary_far_history[i] = s.binary_far_history[i - 1];
    s.far_bit_counts[i] = s.far_bit_counts[i - 1];
  }
  s.binary_far_history[0] = bs;
  s.far_bit_counts[0] = __builtin_popcount(bs);
}
// WebRtc_DelayEstimatorProcessFix + WebRtc_ProcessBinarySpectrum (lookahead 0, robust validation off)
AECM_HD inline int delay_estimator_process(AspAecmState& s, const uint16_t* near, int near_q) {
  const uint32_t bs = binary_spectrum_fix(near, s.mean_near_spectrum, near_q, &s.near_spectrum_initialized);
  s.binary_near_history[0] = bs;
  for (int i = 0; i < kMaxDelay; ++i) {
    s.bit_counts[i] = __builtin_popcount(bs ^ s.binary_far_history[i]);
    if (s.far_bit_counts[i] > 0) {
      const int shifts = 13 - ((3 * s.far_bit_counts[i]) >> 4);
      mean_estimator_fix(s.bit_counts[i] << 9, shifts, &s.mean_bit_counts[i]);
    }
  }
  int32_t best = kMaxBitCountsQ9, worst = 0;
  int cand = -1;
  for (int i = 0; i < kMaxDelay; ++i) {
    if (s.mean_bit_counts[i] < best) {
      best = s.mean_bit_counts[i];
      cand = i;
    }
    if (s.mean_bit_counts[i] > worst) worst = s.mean_bit_counts[i];
  }
  const int32_t valley = worst - best;
  if (s.minimum_probability > 8704 && valley > 2816) {
    int32_t threshold = best + 1024;
    if (threshold < 8704) threshold = 8704;
    if (s.minimum_probability > threshold) s.minimum_probability = threshold;
  }
  s.last_delay_probability++;
  const int valid = valley > 1024 && (best < s.minimum_probability || best < s.last_delay_probability);
  if (valid) {
    s.last_delay = cand;
    if (best < s.last_delay_probability) s.last_delay_probability = best;
    s.compare_delay = s.last_delay;
  }
  return s.last_delay;
}

// ------------------------------------------------------------------ core (aecm_core.c)
AECM_HD inline void init_echo_path_core(AspAecmState& s, const int16_t* ep) {
  for (int i = 0; i < kPartLen1; ++i) {
    s.channelStored[i] = ep[i];
    s.channelAdapt16[i] = ep[i];
    s.channelAdapt32[i] = (int32_t)((uint32_t)(int32_t)ep[i] << 16);
  }
  s.mseAdaptOld = 1000;
  s.mseStoredOld = 1000;
  s.mseThreshold = 0x7FFFFFFF;
  s.mseChannelCount = 0;
}

AECM_HD inline void init_core(AspAecmState& s, int fs, const AecmTables& T) {
  s.mult = (int16_t)(fs / 8000);
  s.farBufWritePos = 0;
  s.farBufReadPos = 0;
  s.coreKnownDelay = 0;
  s.lastKnownDelay = 0;
  ring_init(s.farFrameBuf, s.farFrameBuf_data, kFrameBufLen);
  ring_init(s.nearNoisyFrameBuf, s.nearNoisyFrameBuf_data, kFrameBufLen);
  ring_init(s.nearCleanFrameBuf, s.nearCleanFrameBuf_data, kFrameBufLen);
  ring_init(s.outFrameBuf, s.outFrameBuf_data, kFrameBufLen);
  for (int i = 0; i < 128; ++i) s.xBuf[i] = s.dBufClean[i] = s.dBufNoisy[i] = 0;
  for (int i = 0; i < 64; ++i) s.outBuf[i] = 0;
  s.seed = 666;
  s.totCount = 0;
  // WebRtc_InitDelayEstimatorFarend / WebRtc_InitDelayEstimator
  for (int i = 0; i < kPartLen1; ++i) s.mean_far_spectrum[i] = s.mean_near_spectrum[i] = 0;
  s.far_spectrum_initialized = 0;
  s.near_spectrum_initialized = 0;
  for (int i = 0; i < kMaxDelay; ++i) {
    s.binary_far_history[i] = 0;
    s.far_bit_counts[i] = 0;
    s.bit_counts[i] = 0;
  }
  for (int i = 0; i <= kMaxDelay; ++i) s.mean_bit_counts[i] = 20 << 9;
  s.binary_near_history[0] = 0;
  s.minimum_probability = kMaxBitCountsQ9;
  s.last_delay_probability = kMaxBitCountsQ9;
  s.last_delay = -2;
  s.last_candidate_delay = -2;
  s.compare_delay = kMaxDelay;
  s.candidate_hits = 0;
  for (int i = 0; i < kPartLen1 * kMaxDelay; ++i) s.far_history[i] = 0;
  for (int i = 0; i < kMaxDelay; ++i) s.far_q_domains[i] = 0;
  s.far_history_pos = kMaxDelay;
  s.nlpFlag = 1;
  s.fixedDelay = -1;
  s.dfaCleanQDomain = s.dfaCleanQDomainOld = s.dfaNoisyQDomain = s.dfaNoisyQDomainOld = 0;
  for (int i = 0; i < 64; ++i) s.nearLogEnergy[i] = s.echoAdaptLogEnergy[i] = s.echoStoredLogEnergy[i] = 0;
  s.farLogEnergy = 0;
  init_echo_path_core(s, fs == 8000 ? T.ch8 : T.ch16);
  for (int i = 0; i < kPartLen1; ++i) {
    s.echoFilt[i] = 0;
    s.nearFilt[i] = 0;
    s.noiseEstTooLowCtr[i] = 0;
    s.noiseEstTooHighCtr[i] = 0;
  }
  s.noiseEstCtr = 0;
  s.cngMode = 1;
  int32_t t32 = kPartLen1 * kPartLen1;
  int t16 = kPartLen1;
  int i = 0;
  for (; i < (kPartLen1 >> 1) - 1; ++i) {
    s.noiseEst[i] = t32 << 8;
    --t16;
    t32 -= (t16 << 1) + 1;
  }
  for (; i < kPartLen1; ++i) s.noiseEst[i] = t32 << 8;
  s.farEnergyMin = 32767;
  s.farEnergyMax = -32768;
  s.farEnergyMaxMin = 0;
  s.farEnergyVAD = 1025;
  s.farEnergyMSE = 0;
  s.currentVADValue = 0;
  s.vadUpdateCount = 0;
  s.firstVAD = 1;
  s.startupState = 0;
  s.supGain = 256;
  s.supGainOld = 256;
  s.supGainErrParamA = 3072;
  s.supGainErrParamD = 256;
  s.supGainErrParamDiffAB = 3072 - 1536;
  s.supGainErrParamDiffBD = 1536 - 256;
}

// WebRtcAecm_set_config's state part (the host validates)
AECM_HD inline void set_config(AspAecmState& s, int cngMode, int echoMode) {
  s.cngMode = (int16_t)cngMode;
  s.echoMode = (int16_t)echoMode;
  // mode 0..4: the defaults scaled by 2^(mode - 3)
  const int a = 3072, b = 1536, d = 256;
  int ga, gb, gd;
  if (echoMode < 3) {
    const int sh = 3 - echoMode;
    ga = a >> sh;
    gb = b >> sh;
    gd = d >> sh;
  } else {
    const int sh = echoMode - 3;
    ga = a << sh;
    gb = b << sh;
    gd = d << sh;
  }
  s.supGain = (int16_t)gd;
  s.supGainOld = (int16_t)gd;
  s.supGainErrParamA = (int16_t)ga;
  s.supGainErrParamD = (int16_t)gd;
  s.supGainErrParamDiffAB = (int16_t)(ga - gb);
  s.supGainErrParamDiffBD = (int16_t)(gb - gd);
}

// WebRtcAecm_Init's state part (the host validates the rate)
AECM_HD inline void init_instance(AspAecmState& s, int fs, const AecmTables& T) {
  s.sampFreq = fs;
  init_core(s, fs, T);
  ring_init(s.farendBuf, s.farendBuf_data, kFarendBufLen);
  s.delayChange = 1;
  s.sum = 0;
  s.counter = 0;
  s.checkBuffSize = 1;
  s.firstVal = 0;
  s.ECstartup = 1;
  s.bufSizeStart = 0;
  s.checkBufSizeCtr = 0;
  s.filtDelay = 0;
  s.timeForDelayChange = 0;
  s.knownDelay = 0;
  s.lastDelayDiff = 0;
  for (int i = 0; i < 160; ++i) s.farendOld[i / 80][i % 80] = 0;
  set_config(s, 1, 3);
}

AECM_HD inline int16_t log_energy_q8(uint32_t energy, int q) {
  int v = 7 << 7;
  if (energy > 0) {
    const int zeros = norm_u32(energy);
    const int frac = (int16_t)(((energy << zeros) & 0x7FFFFFFF) >> 23);
    v += ((31 - zeros) << 8) + frac - (q << 8);
  }
  return (int16_t)v;
}
AECM_HD inline int16_t asym_filt(int16_t old, int16_t in, int pos, int neg) {
  if (old == 32767 || old == -32768) return in;
  int16_t r = old;
  if (old > in)
    r = (int16_t)(r - ((old - in) >> neg));
  else
    r = (int16_t)(r + ((in - old) >> pos));
  return r;
}

AECM_HD inline void calc_energies(AspAecmState& s, const uint16_t* far, int far_q, uint32_t nearEner,
                                  int32_t* echoEst) {
  int inc_max = 4, dec_max = 11, inc_min = 11, dec_min = 3;
  for (int i = 63; i > 0; --i) s.nearLogEnergy[i] = s.nearLogEnergy[i - 1];
  s.nearLogEnergy[0] = log_energy_q8(nearEner, s.dfaNoisyQDomain);
  uint32_t tFar = 0, tAdapt = 0, tStored = 0;
  for (int i = 0; i < kPartLen1; ++i) {
    echoEst[i] = (int32_t)s.channelStored[i] * (int32_t)far[i];
    tFar += far[i];
    tAdapt += (uint32_t)((int32_t)s.channelAdapt16[i] * (int32_t)far[i]);
    tStored += (uint32_t)echoEst[i];
  }
  for (int i = 63; i > 0; --i) {
    s.echoAdaptLogEnergy[i] = s.echoAdaptLogEnergy[i - 1];
    s.echoStoredLogEnergy[i] = s.echoStoredLogEnergy[i - 1];
  }
  s.farLogEnergy = log_energy_q8(tFar, far_q);
  s.echoAdaptLogEnergy[0] = log_energy_q8(tAdapt, 12 + far_q);
  s.echoStoredLogEnergy[0] = log_energy_q8(tStored, 12 + far_q);
  if (s.farLogEnergy > 1025) {
    if (s.startupState == 0) {
      inc_max = 2;
      dec_min = 2;
      inc_min = 8;
    }
    s.farEnergyMin = asym_filt(s.farEnergyMin, s.farLogEnergy, inc_min, dec_min);
    s.farEnergyMax = asym_filt(s.farEnergyMax, s.farLogEnergy, inc_max, dec_max);
    s.farEnergyMaxMin = (int16_t)(s.farEnergyMax - s.farEnergyMin);
    int16_t t16 = (int16_t)(2560 - s.farEnergyMin);
    if (t16 > 0)
      t16 = (int16_t)(mul16(t16, 230) >> 9);
    else
      t16 = 0;
    t16 = (int16_t)(t16 + 230);
    if ((s.startupState == 0) | (s.vadUpdateCount > 1024)) {
      s.farEnergyVAD = (int16_t)(s.farEnergyMin + t16);
    } else if (s.farEnergyVAD > s.farLogEnergy) {
      s.farEnergyVAD = (int16_t)(s.farEnergyVAD + ((s.farLogEnergy + t16 - s.farEnergyVAD) >> 6));
      s.vadUpdateCount = 0;
    } else {
      s.vadUpdateCount++;
    }
    s.farEnergyMSE = (int16_t)(s.farEnergyVAD + (1 << 8));
  }
  if (s.farLogEnergy > s.farEnergyVAD) {
    if ((s.startupState == 0) | (s.farEnergyMaxMin > 929)) s.currentVADValue = 1;
  } else {
    s.currentVADValue = 0;
  }
  if (s.currentVADValue && s.firstVAD) {
    s.firstVAD = 0;
    if (s.echoAdaptLogEnergy[0] > s.nearLogEnergy[0]) {
      for (int i = 0; i < kPartLen1; ++i) s.channelAdapt16[i] = (int16_t)(s.channelAdapt16[i] >> 3);
      s.echoAdaptLogEnergy[0] = (int16_t)(s.echoAdaptLogEnergy[0] - (3 << 8));
      s.firstVAD = 1;
    }
  }
}

AECM_HD inline int calc_step_size(const AspAecmState& s) {
  int mu = 1;
  if (!s.currentVADValue) {
    mu = 0;
  } else if (s.startupState > 0) {
    if (s.farEnergyMin >= s.farEnergyMax) {
      mu = 10;
    } else {
      const int16_t t16 = (int16_t)(s.farLogEnergy - s.farEnergyMin);
      int32_t t32 = t16 * 9;
      t32 = div_w32w16(t32, s.farEnergyMaxMin);
      mu = (int16_t)(10 - 1 - (int16_t)t32);
    }
    if (mu < 1) mu = 1;
  }
  return mu;
}

AECM_HD inline void store_adaptive_channel(AspAecmState& s, const uint16_t* far, int32_t* echoEst) {
  for (int i = 0; i < kPartLen1; ++i) {
    s.channelStored[i] = s.channelAdapt16[i];
    echoEst[i] = (int32_t)s.channelStored[i] * (int32_t)far[i];
  }
}
AECM_HD inline void reset_adaptive_channel(AspAecmState& s) {
  for (int i = 0; i < kPartLen1; ++i) {
    s.channelAdapt16[i] = s.channelStored[i];
    s.channelAdapt32[i] = (int32_t)((uint32_t)(int32_t)s.channelStored[i] << 16);
  }
}

AECM_HD inline void update_channel(AspAecmState& s, const uint16_t* far, int far_q, const uint16_t* dfa, int mu,
                                   int32_t* echoEst) {
  if (mu) {
    for (int i = 0; i < kPartLen1; ++i) {
      const int zerosCh = norm_u32((uint32_t)s.channelAdapt32[i]);
      const int zerosFar = norm_u32((uint32_t)far[i]);
      uint32_t u1;
      int shiftChFar;
      if (zerosCh + zerosFar > 31) {
        u1 = (uint32_t)s.channelAdapt32[i] * (uint32_t)far[i];
        shiftChFar = 0;
      } else {
        shiftChFar = 32 - zerosCh - zerosFar;
        u1 = (uint32_t)(s.channelAdapt32[i] >> shiftChFar) * (uint32_t)far[i];
      }
      int zerosNum = norm_u32(u1);
      const int zerosDfa = dfa[i] ? norm_u32((uint32_t)dfa[i]) : 32;
      const int16_t t16 = (int16_t)(zerosDfa - 2 + s.dfaNoisyQDomain - 28 - far_q + shiftChFar);
      int16_t xfaQ, dfaQ;
      if (zerosNum > t16 + 1) {
        xfaQ = t16;
        dfaQ = (int16_t)(zerosDfa - 2);
      } else {
        xfaQ = (int16_t)(zerosNum - 2);
        dfaQ = (int16_t)(28 + far_q - s.dfaNoisyQDomain - shiftChFar + xfaQ);
      }
      u1 = shift_u32(u1, xfaQ);
      const uint32_t u2 = shift_u32((uint32_t)dfa[i], dfaQ);
      const int32_t t1 = (int32_t)(u2 - u1);
      zerosNum = norm_w32(t1);
      if (t1 && (far[i] > (16 << far_q))) {
        int32_t t2;
        int shiftNum;
        if (zerosNum + zerosFar > 31) {
          if (t1 > 0)
            t2 = (int32_t)((uint32_t)t1 * (uint32_t)far[i]);
          else
            t2 = (int32_t)(0u - (0u - (uint32_t)t1) * (uint32_t)far[i]);
          shiftNum = 0;
        } else {
          shiftNum = 32 - (zerosNum + zerosFar);
          if (t1 > 0)
            t2 = (int32_t)((uint32_t)(t1 >> shiftNum) * (uint32_t)far[i]);
          else
            t2 = (int32_t)(0u - (uint32_t)(((int32_t)(0u - (uint32_t)t1)) >> shiftNum) * (uint32_t)far[i]);
        }
        t2 = div_w32w16(t2, i + 1);
        const int shift2 = shiftNum + shiftChFar - xfaQ - mu - ((30 - zerosFar) << 1);
        if (norm_w32(t2) < shift2)
          t2 = 0x7FFFFFFF;
        else
          t2 = shift_w32(t2, shift2);
        s.channelAdapt32[i] = add_sat_w32(s.channelAdapt32[i], t2);
        if (s.channelAdapt32[i] < 0) s.channelAdapt32[i] = 0;
        s.channelAdapt16[i] = (int16_t)(s.channelAdapt32[i] >> 16);
      }
    }
  }
  if ((s.startupState == 0) & (s.currentVADValue != 0)) {
    store_adaptive_channel(s, far, echoEst);
  } else {
    if (s.farLogEnergy < s.farEnergyMSE)
      s.mseChannelCount = 0;
    else
      s.mseChannelCount++;
    if (s.mseChannelCount >= 20 + 10) {
      int32_t mseStored = 0, mseAdapt = 0;
      for (int i = 0; i < 20; ++i) {
        int32_t d = (int32_t)s.echoStoredLogEnergy[i] - (int32_t)s.nearLogEnergy[i];
        mseStored += d >= 0 ? d : -d;
        d = (int32_t)s.echoAdaptLogEnergy[i] - (int32_t)s.nearLogEnergy[i];
        mseAdapt += d >= 0 ? d : -d;
      }
      if (((mseStored << 5) < (29 * mseAdapt)) & ((s.mseStoredOld << 5) < (29 * s.mseAdaptOld))) {
        reset_adaptive_channel(s);
      } else if (((29 * mseStored) > (mseAdapt << 5)) & (mseAdapt < s.mseThreshold) &
                 (s.mseAdaptOld < s.mseThreshold)) {
        store_adaptive_channel(s, far, echoEst);
        if (s.mseThreshold == 0x7FFFFFFF)
          s.mseThreshold = mseAdapt + s.mseAdaptOld;
        else
          s.mseThreshold += mul16(mseAdapt - (mul16(s.mseThreshold, 5) >> 3), 205) >> 8;
      }
      s.mseChannelCount = 0;
      s.mseStoredOld = mseStored;
      s.mseAdaptOld = mseAdapt;
    }
  }
}

AECM_HD inline int16_t calc_suppression_gain(AspAecmState& s) {
  int16_t supGain = 256;
  if (!s.currentVADValue) {
    supGain = 0;
  } else {
    const int16_t t16 = (int16_t)(s.nearLogEnergy[0] - s.echoStoredLogEnergy[0]);
    const int16_t dE = abs_w16(t16);
    if (dE < 400) {
      if (dE < 200) {
        int32_t t32 = s.supGainErrParamDiffAB * dE + 100;
        supGain = (int16_t)(s.supGainErrParamA - (int16_t)div_w32w16(t32, 200));
      } else {
        int32_t t32 = s.supGainErrParamDiffBD * (400 - dE) + 100;
        supGain = (int16_t)(s.supGainErrParamD + (int16_t)div_w32w16(t32, 200));
      }
    } else {
      supGain = s.supGainErrParamD;
    }
  }
  const int16_t t = supGain > s.supGainOld ? supGain : s.supGainOld;
  s.supGainOld = supGain;
  s.supGain = (int16_t)(s.supGain + (int16_t)((t - s.supGain) >> 4));
  return s.supGain;
}

// TimeToFrequencyDomain (AECM_DYNAMIC_Q, SqrtFloor magnitude): 128 samples -> freq [65] (re, im), abs [65]
AECM_HD inline int time_to_freq(const int16_t* time, int16_t* freq, uint16_t* fabs, uint32_t* sum, int16_t* cb,
                                const AecmTables& T) {
  const int scaling = norm_w16(max_abs_w16(time, 128));
  // WindowAndFFT + WebRtcSpl_RealForwardFFT: real input, zero imaginary parts
  for (int i = 0; i < 64; ++i) {
    cb[2 * i] = (int16_t)(mul16((int16_t)(time[i] << scaling), T.hann[i]) >> 14);
    cb[2 * i + 1] = 0;
    cb[2 * (64 + i)] = (int16_t)(mul16((int16_t)(time[64 + i] << scaling), T.hann[64 - i]) >> 14);
    cb[2 * (64 + i) + 1] = 0;
  }
  bit_reverse(cb);
  complex_fft(cb, T.sin1024);
  for (int i = 0; i < 130; ++i) freq[i] = cb[i];
  for (int i = 0; i < 64; ++i) freq[2 * i + 1] = (int16_t)(-freq[2 * i + 1]);
  freq[1] = 0;
  freq[129] = 0;
  fabs[0] = (uint16_t)abs_w16(freq[0]);
  fabs[64] = (uint16_t)abs_w16(freq[128]);
  uint32_t acc = (uint32_t)fabs[0] + (uint32_t)fabs[64];
  for (int i = 1; i < 64; ++i) {
    const int16_t re = freq[2 * i], im = freq[2 * i + 1];
    if (re == 0) {
      fabs[i] = (uint16_t)abs_w16(im);
    } else if (im == 0) {
      fabs[i] = (uint16_t)abs_w16(re);
    } else {
      const int16_t a = abs_w16(re), b = abs_w16(im);
      const int32_t p = add_sat_w32((int32_t)a * a, (int32_t)b * b);
      fabs[i] = (uint16_t)sqrt_floor(p);
    }
    acc += fabs[i];
  }
  *sum = acc;
  return scaling;
}

AECM_HD inline void comfort_noise(AspAecmState& s, AecmWork& w, const uint16_t* dfa, const AecmTables& T) {
  const int shiftN = 15 - s.dfaCleanQDomain;
  int minTrackShift;
  if (s.noiseEstCtr < 100) {
    s.noiseEstCtr++;
    minTrackShift = 6;
  } else {
    minTrackShift = 9;
  }
  for (int i = 0; i < kPartLen1; ++i) {
    const int32_t outL = (int32_t)((uint32_t)dfa[i] << shiftN);
    int32_t ne = s.noiseEst[i];
    if (outL < ne) {
      s.noiseEstTooLowCtr[i] = 0;
      if (ne < (1 << minTrackShift)) {
        s.noiseEstTooHighCtr[i]++;
        if (s.noiseEstTooHighCtr[i] >= 5) {
          ne--;
          s.noiseEstTooHighCtr[i] = 0;
        }
      } else {
        ne -= (int32_t)((uint32_t)ne - (uint32_t)outL) >> minTrackShift;
      }
    } else {
      s.noiseEstTooHighCtr[i] = 0;
      if ((ne >> 19) > 0) {
        ne >>= 11;
        ne *= 2049;
      } else if ((ne >> 11) > 0) {
        ne *= 2049;
        ne >>= 11;
      } else {
        s.noiseEstTooLowCtr[i]++;
        if (s.noiseEstTooLowCtr[i] >= 5) {
          ne += (ne >> 9) + 1;
          s.noiseEstTooLowCtr[i] = 0;
        }
      }
    }
    s.noiseEst[i] = ne;
  }
  int16_t* nr = w.noiseR;
  for (int i = 0; i < kPartLen1; ++i) {
    int32_t t32 = s.noiseEst[i] >> shiftN;
    if (t32 > 32767) {
      t32 = 32767;
      s.noiseEst[i] = t32 << shiftN;
    }
    const int16_t t16 = (int16_t)(16384 - w.hnl[i]);
    nr[i] = (int16_t)(mul16(t16, (int16_t)t32) >> 14);
  }
  uint32_t seed = s.seed;
  for (int i = 1; i < kPartLen1; ++i) {
    seed = (seed * 69069u + 1u) & 0x7FFFFFFFu;
    const int16_t r = (int16_t)(seed >> 16);
    const int16_t t16 = (int16_t)(mul16(359, r) >> 15);
    const int16_t ur = (int16_t)(mul16(nr[i], T.cos360[t16]) >> 13);
    const int16_t ui = i == kPartLen ? (int16_t)0 : (int16_t)(mul16(-nr[i], T.sin360[t16]) >> 13);
    w.efw[2 * i] = sat_w16((int32_t)w.efw[2 * i] + ur);
    w.efw[2 * i + 1] = sat_w16((int32_t)w.efw[2 * i + 1] + ui);
  }
  s.seed = seed;
}

AECM_HD inline void inverse_fft_and_window(AspAecmState& s, AecmWork& w, int16_t* output, bool clean,
                                           const AecmTables& T) {
  int16_t* cb = w.cb;
  // fft[0..129] from efw (conjugated), then RealInverseFFT's mirror of the upper half
  for (int i = 0; i < 65; ++i) {
    cb[2 * i] = w.efw[2 * i];
    cb[2 * i + 1] = (int16_t)(-w.efw[2 * i + 1]);
  }
  for (int i = 130; i < 256; i += 2) {
    cb[i] = cb[256 - i];
    cb[i + 1] = (int16_t)(-cb[256 - i + 1]);
  }
  bit_reverse(cb);
  const int outCFFT = complex_ifft(cb, T.sin1024);
  const int sh = outCFFT - s.dfaCleanQDomain;
  for (int i = 0; i < 64; ++i) {
    const int16_t a = (int16_t)((mul16(cb[2 * i], T.hann[i]) + 8192) >> 14);
    int32_t t32 = shift_w32((int32_t)a, sh);
    output[i] = sat_w16(t32 + s.outBuf[i]);
    t32 = mul16(cb[2 * (64 + i)], T.hann[64 - i]) >> 14;
    t32 = shift_w32(t32, sh);
    s.outBuf[i] = sat_w16(t32);
  }
  for (int i = 0; i < 64; ++i) {
    s.xBuf[i] = s.xBuf[64 + i];
    s.dBufNoisy[i] = s.dBufNoisy[64 + i];
    if (clean) s.dBufClean[i] = s.dBufClean[64 + i];
  }
}

AECM_HD inline void process_block(AspAecmState& s, AecmWork& w, const int16_t* farend, const int16_t* nearN,
                                  const int16_t* nearC, int16_t* output, const AecmTables& T) {
  if (s.startupState < 2) s.startupState = (int16_t)((s.totCount >= 512) + (s.totCount >= 1024));
  for (int i = 0; i < 64; ++i) {
    s.xBuf[64 + i] = farend[i];
    s.dBufNoisy[64 + i] = nearN[i];
    if (nearC) s.dBufClean[64 + i] = nearC[i];
  }
  uint32_t xfaSum, dfaNoisySum, dfaCleanSum;
  const int far_q0 = time_to_freq(s.xBuf, w.dfw, w.xfa, &xfaSum, w.cb, T);
  const int zerosN = time_to_freq(s.dBufNoisy, w.dfw, w.dfaN, &dfaNoisySum, w.cb, T);
  s.dfaNoisyQDomainOld = s.dfaNoisyQDomain;
  s.dfaNoisyQDomain = (int16_t)zerosN;
  const uint16_t* dfaC;
  if (!nearC) {
    dfaC = w.dfaN;
    s.dfaCleanQDomainOld = s.dfaNoisyQDomainOld;
    s.dfaCleanQDomain = s.dfaNoisyQDomain;
    dfaCleanSum = dfaNoisySum;
  } else {
    const int zc = time_to_freq(s.dBufClean, w.dfw, w.dfaC, &dfaCleanSum, w.cb, T);
    s.dfaCleanQDomainOld = s.dfaCleanQDomain;
    s.dfaCleanQDomain = (int16_t)zc;
    dfaC = w.dfaC;
  }
  (void)dfaCleanSum;
  // UpdateFarHistory
  if (++s.far_history_pos >= kMaxDelay) s.far_history_pos = 0;
  s.far_q_domains[s.far_history_pos] = far_q0;
  for (int i = 0; i < kPartLen1; ++i) s.far_history[s.far_history_pos * kPartLen1 + i] = w.xfa[i];
  add_far_spectrum(s, w.xfa, far_q0);
  int delay = delay_estimator_process(s, w.dfaN, zerosN);
  if (delay == -2) delay = 0;
  if (s.fixedDelay >= 0) delay = s.fixedDelay;
  // AlignedFarend
  int pos = s.far_history_pos - delay;
  if (pos < 0) pos += kMaxDelay;
  const int far_q = s.far_q_domains[pos];
  const uint16_t* farSp = &s.far_history[pos * kPartLen1];
  const int16_t zerosXBuf = (int16_t)far_q;
  int32_t* echoEst = w.echoEst;
  calc_energies(s, farSp, zerosXBuf, dfaNoisySum, echoEst);
  const int mu = calc_step_size(s);
  s.totCount++;
  update_channel(s, farSp, zerosXBuf, w.dfaN, mu, echoEst);
  const int16_t supGain = calc_suppression_gain(s);
  int16_t* hnl = w.hnl;
  int numPosCoef = 0;
  for (int i = 0; i < kPartLen1; ++i) {
    const int32_t d = (int32_t)((uint32_t)echoEst[i] - (uint32_t)s.echoFilt[i]);
    s.echoFilt[i] = (int32_t)((uint32_t)s.echoFilt[i] + (uint32_t)((int32_t)((uint32_t)d * 50u) >> 8));
    const int zeros32 = norm_w32(s.echoFilt[i]) + 1;
    const int zeros16 = norm_w16(supGain) + 1;
    uint32_t gained;
    int16_t resDiff;
    if (zeros32 + zeros16 > 16) {
      gained = (uint32_t)s.echoFilt[i] * (uint32_t)(uint16_t)supGain;
      resDiff = (int16_t)(14 - 12 - 8 + (s.dfaCleanQDomain - zerosXBuf));
    } else {
      const int t = 17 - zeros32 - zeros16;
      resDiff = (int16_t)(14 + t - 12 - 8 + (s.dfaCleanQDomain - zerosXBuf));
      if (zeros32 > t)
        gained = (uint32_t)s.echoFilt[i] * (uint32_t)(uint16_t)(supGain >> t);
      else
        gained = (uint32_t)(s.echoFilt[i] >> t) * (uint32_t)(int32_t)supGain;
    }
    const int z16 = norm_w16(s.nearFilt[i]);
    const int16_t qdd = (int16_t)(s.dfaCleanQDomain - s.dfaCleanQDomainOld);
    int16_t a16, b16, qDomainDiff;
    if (z16 < qdd && s.nearFilt[i]) {
      a16 = (int16_t)(s.nearFilt[i] << z16);
      qDomainDiff = (int16_t)(z16 - qdd);
      b16 = (int16_t)(dfaC[i] >> -qDomainDiff);
    } else {
      a16 = qdd < 0 ? (int16_t)(s.nearFilt[i] >> -qdd) : (int16_t)(s.nearFilt[i] << qdd);
      qDomainDiff = 0;
      b16 = (int16_t)dfaC[i];
    }
    const int32_t t32 = (int32_t)(b16 - a16);
    b16 = (int16_t)(t32 >> 4);
    b16 = (int16_t)(b16 + a16);
    const int zz = norm_w16(b16);
    if (b16 & (int)(-qDomainDiff > zz))
      s.nearFilt[i] = 32767;
    else
      s.nearFilt[i] = qDomainDiff < 0 ? (int16_t)(b16 << -qDomainDiff) : (int16_t)(b16 >> qDomainDiff);
    if (gained == 0) {
      hnl[i] = 16384;
    } else if (s.nearFilt[i] == 0) {
      hnl[i] = 0;
    } else {
      gained += (uint32_t)(s.nearFilt[i] >> 1);
      const uint32_t q = div_u32u16(gained, (uint16_t)s.nearFilt[i]);
      const int32_t r = (int32_t)shift_u32(q, resDiff);
      if (r > 16384)
        hnl[i] = 0;
      else if (r < 0)
        hnl[i] = 16384;
      else {
        hnl[i] = (int16_t)(16384 - (int16_t)r);
        if (hnl[i] < 0) hnl[i] = 0;
      }
    }
    if (hnl[i]) numPosCoef++;
  }
  if (s.mult == 2) {
    for (int i = 0; i < kPartLen1; ++i) hnl[i] = (int16_t)(mul16(hnl[i], hnl[i]) >> 14);
    int32_t avg = 0;
    for (int i = 4; i <= 24; ++i) avg += hnl[i];
    avg /= 21;
    for (int i = 24; i < kPartLen1; ++i)
      if (hnl[i] > (int16_t)avg) hnl[i] = (int16_t)avg;
  }
  for (int i = 0; i < kPartLen1; ++i) {
    if (s.nlpFlag) {
      if (hnl[i] > 16384)
        hnl[i] = 16384;
      else if (hnl[i] < 3277)
        hnl[i] = 0;
      const int nlpGain = numPosCoef < 3 ? 0 : 16384;
      if (!(hnl[i] == 16384 && nlpGain == 16384)) hnl[i] = (int16_t)(mul16(hnl[i], nlpGain) >> 14);
    }
    w.efw[2 * i] = (int16_t)((mul16(w.dfw[2 * i], hnl[i]) + 8192) >> 14);
    w.efw[2 * i + 1] = (int16_t)((mul16(w.dfw[2 * i + 1], hnl[i]) + 8192) >> 14);
  }
  if (s.cngMode == 1) comfort_noise(s, w, dfaC, T);
  inverse_fft_and_window(s, w, output, nearC != nullptr, T);
}

// WebRtcAecm_ProcessFrame: 80 samples in, 80 out
AECM_HD inline void process_frame(AspAecmState& s, AecmWork& w, const int16_t* farend, const int16_t* nearN,
                                  const int16_t* nearC, int16_t* out, const AecmTables& T) {
  // BufferFarFrame into farBuf, FetchFarFrame with the core's knownDelay
  {
    int len = 80, wp = 0;
    while (s.farBufWritePos + len > kFarBufLen) {
      len = kFarBufLen - s.farBufWritePos;
      for (int i = 0; i < len; ++i) s.farBuf[s.farBufWritePos + i] = farend[wp + i];
      s.farBufWritePos = 0;
      wp = len;
      len = 80 - len;
    }
    for (int i = 0; i < len; ++i) s.farBuf[s.farBufWritePos + i] = farend[wp + i];
    s.farBufWritePos += len;
  }
  {
    int len = 80, rp = 0;
    s.farBufReadPos -= s.coreKnownDelay - s.lastKnownDelay;
    while (s.farBufReadPos < 0) s.farBufReadPos += kFarBufLen;
    while (s.farBufReadPos > kFarBufLen - 1) s.farBufReadPos -= kFarBufLen;
    s.lastKnownDelay = s.coreKnownDelay;
    while (s.farBufReadPos + len > kFarBufLen) {
      len = kFarBufLen - s.farBufReadPos;
      for (int i = 0; i < len; ++i) w.farFrame[rp + i] = s.farBuf[s.farBufReadPos + i];
      s.farBufReadPos = 0;
      rp = len;
      len = 80 - len;
    }
    for (int i = 0; i < len; ++i) w.farFrame[rp + i] = s.farBuf[s.farBufReadPos + i];
    s.farBufReadPos += len;
  }
  ring_write(s.farFrameBuf, s.farFrameBuf_data, kFrameBufLen, w.farFrame, 80);
  ring_write(s.nearNoisyFrameBuf, s.nearNoisyFrameBuf_data, kFrameBufLen, nearN, 80);
  if (nearC) ring_write(s.nearCleanFrameBuf, s.nearCleanFrameBuf_data, kFrameBufLen, nearC, 80);
  while (ring_avail_read(s.farFrameBuf, kFrameBufLen) >= 64) {
    ring_read(s.farFrameBuf, s.farFrameBuf_data, kFrameBufLen, w.blkFar, 64);
    ring_read(s.nearNoisyFrameBuf, s.nearNoisyFrameBuf_data, kFrameBufLen, w.blkNear, 64);
    if (nearC) ring_read(s.nearCleanFrameBuf, s.nearCleanFrameBuf_data, kFrameBufLen, w.blkClean, 64);
    process_block(s, w, w.blkFar, w.blkNear, nearC ? w.blkClean : nullptr, w.outBlock, T);
    ring_write(s.outFrameBuf, s.outFrameBuf_data, kFrameBufLen, w.outBlock, 64);
  }
  const int size = ring_avail_read(s.outFrameBuf, kFrameBufLen);
  if (size < 80) ring_move(s.outFrameBuf, kFrameBufLen, size - 80);
  ring_read(s.outFrameBuf, s.outFrameBuf_data, kFrameBufLen, out, 80);
}

// WebRtcAecm_BufferFarend after validation
AECM_HD inline void buffer_farend(AspAecmState& s, const int16_t* farend, int n) {
  if (!s.ECstartup) {  // WebRtcAecm_DelayComp
    const int nSampFar = ring_avail_read(s.farendBuf, kFarendBufLen);
    const int nSampSndCard = s.msInSndCardBuf * 8 * s.mult;
    const int delayNew = nSampSndCard - nSampFar;
    if (delayNew > kFarBufLen - 80 * s.mult) {
      int add = (nSampSndCard >> 1) - nSampFar;
      if (add < 80) add = 80;
      if (add > 800) add = 800;
      ring_move(s.farendBuf, kFarendBufLen, -add);
      s.delayChange = 1;
    }
  }
  ring_write(s.farendBuf, s.farendBuf_data, kFarendBufLen, farend, n);
}

AECM_HD inline void est_buf_delay(AspAecmState& s) {
  const int16_t nSampFar = (int16_t)ring_avail_read(s.farendBuf, kFarendBufLen);
  const int16_t nSampSndCard = (int16_t)(s.msInSndCardBuf * 8 * s.mult);
  int16_t delayNew = (int16_t)(nSampSndCard - nSampFar);
  if (delayNew < 80) {
    ring_move(s.farendBuf, kFarendBufLen, 80);
    delayNew = (int16_t)(delayNew + 80);
  }
  const int fd = (8 * s.filtDelay + 2 * delayNew) / 10;
  s.filtDelay = (int16_t)(fd > 0 ? fd : 0);
  const int16_t diff = (int16_t)(s.filtDelay - s.knownDelay);
  if (diff > 224) {
    if (s.lastDelayDiff < 96)
      s.timeForDelayChange = 0;
    else
      s.timeForDelayChange++;
  } else if (diff < 96 && s.knownDelay > 0) {
    if (s.lastDelayDiff > 224)
      s.timeForDelayChange = 0;
    else
      s.timeForDelayChange++;
  } else {
    s.timeForDelayChange = 0;
  }
  s.lastDelayDiff = diff;
  if (s.timeForDelayChange > 25) {
    const int k = (int)s.filtDelay - 160;
    s.knownDelay = k > 0 ? k : 0;
  }
}

// WebRtcAecm_Process after validation; ms is the clamped msInSndCardBuf
AECM_HD inline void process(AspAecmState& s, AecmWork& w, const int16_t* nearN, const int16_t* nearC, int16_t* out,
                            int n, int ms, const AecmTables& T) {
  s.msInSndCardBuf = (int16_t)(ms + 10);
  const int nFrames = n / 80;
  const int nBlocks10ms = nFrames / s.mult;
  if (s.ECstartup) {
    const int16_t* src = nearC ? nearC : nearN;
    if (out != src)
      for (int i = 0; i < n; ++i) out[i] = src[i];
    const int filled = (int16_t)ring_avail_read(s.farendBuf, kFarendBufLen) / 80;
    if (s.checkBuffSize) {
      s.checkBufSizeCtr++;
      if (s.counter == 0) {
        s.firstVal = s.msInSndCardBuf;
        s.sum = 0;
      }
      const int dv = s.firstVal - s.msInSndCardBuf;
      const double lim = 0.2 * s.msInSndCardBuf > 8 ? 0.2 * s.msInSndCardBuf : 8;
      if ((dv < 0 ? -dv : dv) < lim) {
        s.sum = (int16_t)(s.sum + s.msInSndCardBuf);
        s.counter++;
      } else {
        s.counter = 0;
      }
      if (s.counter * nBlocks10ms >= 6) {
        const int v = (3 * s.sum * s.mult) / (s.counter * 40);
        s.bufSizeStart = (int16_t)(v < 50 ? v : 50);
        s.checkBuffSize = 0;
      }
      if (s.checkBufSizeCtr * nBlocks10ms > 50) {
        const int v = (3 * s.msInSndCardBuf * s.mult) / 40;
        s.bufSizeStart = (int16_t)(v < 50 ? v : 50);
        s.checkBuffSize = 0;
      }
    }
    if (!s.checkBuffSize) {
      if (filled == s.bufSizeStart) {
        s.ECstartup = 0;
      } else if (filled > s.bufSizeStart) {
        ring_move(s.farendBuf, kFarendBufLen,
                  ring_avail_read(s.farendBuf, kFarendBufLen) - (int)s.bufSizeStart * 80);
        s.ECstartup = 0;
      }
    }
  } else {
    for (int i = 0; i < nFrames; ++i) {
      const int filled = (int16_t)ring_avail_read(s.farendBuf, kFarendBufLen) / 80;
      if (filled > 0) {
        ring_read(s.farendBuf, s.farendBuf_data, kFarendBufLen, w.farend, 80);
        for (int k = 0; k < 80; ++k) s.farendOld[i][k] = w.farend[k];
      } else {
        for (int k = 0; k < 80; ++k) w.farend[k] = s.farendOld[i][k];
      }
      if ((i == 0 && s.sampFreq == 8000) || (i == 1 && s.sampFreq == 16000)) est_buf_delay(s);
      process_frame(s, w, w.farend, nearN + 80 * i, nearC ? nearC + 80 * i : nullptr, out + 80 * i, T);
    }
  }
}

}  // namespace aspaecm
#endif  // ASP_AECM_CORE_H_
