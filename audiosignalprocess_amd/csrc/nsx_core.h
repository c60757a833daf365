// nsx_core.h -- one stream of the fixed-point noise suppressor, restated with the reference's integer
// semantics (noise_suppression_x.c, nsx_core.c, nsx_core_c.c and the spl helpers they call).
//
// One source for two builds.  Every per-bin loop is written "for (i = L.id; i < n; i += L.n)" and every
// cross-bin quantity goes through wsum / wmax / wmin:
//   * the kernel (nsx_kernels.hip) runs it with one wave per stream, L = {lane, 64}: bin q, q + 64 and
//     the bin-128 tail sit on lane q, the reductions are wave reductions, wsync() orders one lane's
//     stores before another lane's loads (a fence, no workgroup barrier);
//   * the CPU build (nsx_restate.cpp) runs it with L = {0, 1}: plain loops, reductions are the identity.
// The wrapping int32 / uint32 sums are associative mod 2^32 and maxima are order-free, so both builds
// give the reference's bits.  Wave-uniform scalar steps (feature update, histograms, parameter
// extraction, the pink-noise fit) run on lane 0.  Signed wrap is written as unsigned arithmetic.
#ifndef ASP_NSX_CORE_H_
#define ASP_NSX_CORE_H_

#include "nsx_layout.h"

namespace aspnsx {

struct Lanes {
  int id, n;
};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ inline uint32_t wsum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}
__device__ inline int32_t wmax(int32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const int32_t t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ inline int32_t wmin(int32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const int32_t t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ inline uint32_t wmaxu(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
#else
NSX_HD inline void wsync() {}
NSX_HD inline uint32_t wsum(uint32_t v) { return v; }
NSX_HD inline int32_t wmax(int32_t v) { return v; }
NSX_HD inline int32_t wmin(int32_t v) { return v; }
NSX_HD inline uint32_t wmaxu(uint32_t v) { return v; }
#endif

// ------------------------------------------------------------------ spl helpers (spl_inl.h, *.c)
NSX_HD inline int norm_u32(uint32_t a) { return a == 0 ? 0 : __builtin_clz(a); }
NSX_HD inline int norm_w32(int32_t a) {
  if (a == 0) return 0;
  const uint32_t u = (uint32_t)(a < 0 ? ~a : a);
  return u == 0 ? 31 : __builtin_clz(u) - 1;
}
NSX_HD inline int norm_w16(int a16) {
  const int32_t a = (int16_t)a16;
  if (a == 0) return 0;
  const uint32_t u = (uint32_t)(a < 0 ? ~a : a);
  return u == 0 ? 15 : __builtin_clz(u) - 17;
}
NSX_HD inline int16_t sat_w16(int32_t v) { return (int16_t)(v > 32767 ? 32767 : v < -32768 ? -32768 : v); }
NSX_HD inline int16_t add_sat_w16(int16_t a, int16_t b) { return sat_w16((int32_t)a + (int32_t)b); }
NSX_HD inline int32_t div_w32w16(int32_t num, int den16) {
  const int16_t den = (int16_t)den16;
  if (den == 0) return 0x7FFFFFFF;
  if (den == -1) return (int32_t)(0u - (uint32_t)num);
  return num / den;
}
NSX_HD inline uint32_t div_u32u16(uint32_t num, uint16_t den) { return den != 0 ? num / den : 0xFFFFFFFFu; }
NSX_HD inline int32_t sqrt_floor(int32_t value) {
  int32_t root = 0;
  for (int n = 15; n >= 0; --n) {
    const int32_t t = (int32_t)((uint32_t)(root + (1 << n)) << n);
    if (value >= t) {
      value -= t;
      root |= 2 << n;
    }
  }
  return root >> 1;
}
// WEBRTC_SPL_SHIFT_W32 (left shifts as unsigned: defined wrap)
NSX_HD inline int32_t shift_w32(int32_t x, int c) { return c >= 0 ? (int32_t)((uint32_t)x << c) : x >> -c; }
NSX_HD inline int32_t mul16(int a, int b) { return (int32_t)(int16_t)a * (int32_t)(int16_t)b; }
NSX_HD inline int32_t mul16_rsft_round(int a, int b, int c) { return (mul16(a, b) + (1 << (c - 1))) >> c; }
NSX_HD inline int32_t wrap_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
NSX_HD inline int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
NSX_HD inline int32_t wrap_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
// 256 log2(m) in Q8 from the fraction table, 0 for m == 0 where the caller says so
NSX_HD inline int log2_q8(uint32_t m, const NsxTables& T) {
  const int zeros = norm_u32(m);
  const int frac = (int)(((m << zeros) & 0x7FFFFFFF) >> 23);
  return ((31 - zeros) << 8) + T.logFrac[frac];
}

// ------------------------------------------------------------------ Init / set_policy (nsx_core.c)
NSX_HD inline int set_policy_core(AspNsxState& s, int mode) {
  if (mode < 0 || mode > 3) return -1;
  static const uint16_t od[4] = {256, 256, 282, 320}, db[4] = {8192, 4096, 2048, 1475};
  s.aggrMode = mode;
  s.overdrive = mode == 0 ? 256 : mode == 1 ? 256 : mode == 2 ? 282 : 320;
  s.denoiseBound = mode == 0 ? 8192 : mode == 1 ? 4096 : mode == 2 ? 2048 : 1475;
  s.gainMap = mode != 0;
  (void)od;
  (void)db;
  return 0;
}
// WebRtcNsx_InitCore.  real, imag, normData and the two energyIn fields' neighbours keep their values,
// as in the reference (it does not touch them).
NSX_HD inline int init_core(AspNsxState& s, uint32_t fs) {
  if (fs != 8000 && fs != 16000 && fs != 32000 && fs != 48000) return -1;
  s.fs = fs;
  if (fs == 8000) {
    s.blockLen10ms = 80;
    s.anaLen = 128;
    s.stages = 7;
    s.thresholdLogLrt = 131072;
    s.maxLrt = 0x0040000;
    s.minLrt = 52429;
  } else {
    s.blockLen10ms = 160;
    s.anaLen = 256;
    s.stages = 8;
    s.thresholdLogLrt = 212644;
    s.maxLrt = 0x0080000;
    s.minLrt = 104858;
  }
  s.anaLen2 = s.anaLen / 2;
  s.magnLen = s.anaLen2 + 1;
  for (int i = 0; i < 256; ++i) s.analysisBuffer[i] = s.synthesisBuffer[i] = s.dataBufHBFX[0][i] = s.dataBufHBFX[1][i] = 0;
  for (int i = 0; i < 3 * 129; ++i) {
    s.noiseEstLogQuantile[i] = 2048;
    s.noiseEstDensity[i] = 153;
  }
  for (int i = 0; i < 3; ++i) s.noiseEstCounter[i] = (int16_t)((int16_t)(200 * (i + 1)) / 3);
  for (int i = 0; i < 129; ++i) {
    s.noiseEstQuantile[i] = 0;
    s.noiseSupFilter[i] = 16384;
    s.prevMagnU16[i] = 0;
    s.prevNoiseU32[i] = 0;
    s.logLrtTimeAvgW32[i] = 0;
    s.avgMagnPause[i] = 0;
    s.initMagnEst[i] = 0;
  }
  s.aggrMode = 0;
  s.priorNonSpeechProb = 8192;
  s.thresholdSpecDiff = 50;
  s.thresholdSpecFlat = 20480;
  s.featureLogLrt = s.thresholdLogLrt;
  s.featureSpecFlat = s.thresholdSpecFlat;
  s.featureSpecDiff = s.thresholdSpecDiff;
  s.weightLogLrt = 6;
  s.weightSpecFlat = 0;
  s.weightSpecDiff = 0;
  s.curAvgMagnEnergy = s.timeAvgMagnEnergy = s.timeAvgMagnEnergyTmp = 0;
  for (int i = 0; i < kHist; ++i) s.histLrt[i] = s.histSpecDiff[i] = s.histSpecFlat[i] = 0;
  s.blockIndex = -1;
  s.modelUpdate = 1 << 9;
  s.cntThresUpdate = 0;
  s.sumMagn = s.magnEnergy = 0;
  s.prevQMagn = s.qNoise = s.prevQNoise = 0;
  s.energyIn = s.scaleEnergyIn = 0;
  s.whiteNoiseLevel = 0;
  s.pinkNoiseNumerator = s.pinkNoiseExp = 0;
  s.minNorm = 15;
  s.zeroInputSignal = 0;
  set_policy_core(s, 0);
  s.initFlag = 1;
  return 0;
}

// ------------------------------------------------------------------ complex FFT across the lanes
NSX_HD inline int bitrev(int i, int stages) {
  int r = 0;
  for (int b = 0; b < stages; ++b) r |= ((i >> b) & 1) << (stages - 1 - b);
  return r;
}
// WebRtcSpl_ComplexFFT (mode 1) / ComplexIFFT (mode 1) on a bit-reversed buffer of n = 1 << stages points.
// One butterfly per lane and step: the n / 2 butterflies of a stage touch disjoint pairs, so any order
// gives complex_fft.c's values; a wsync() between stages.  The inverse picks each stage's shift from the
// max-abs of the whole buffer (a wave max).  Returns the inverse's total scale (0 for the forward).
NSX_HD inline int complex_fft(int16_t* fr, int stages, bool inverse, const NsxTables& T, Lanes L) {
  const int n = 1 << stages;
  int scale = 0, k = 9, lg = 0;
  for (int l = 1; l < n; l <<= 1, --k, ++lg) {
    int shift = 1;
    int32_t round2 = 16384;
    if (inverse) {
      int32_t mx = 0;
      for (int i = L.id; i < 2 * n; i += L.n) {
        const int32_t a = fr[i] < 0 ? -(int32_t)fr[i] : (int32_t)fr[i];
        mx = a > mx ? a : mx;
      }
      mx = wmax(mx);
      if (mx > 32767) mx = 32767;
      shift = 0;
      round2 = 8192;
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
    }
    for (int b = L.id; b < n / 2; b += L.n) {
      const int m = b & (l - 1);
      const int i = ((b >> lg) << (lg + 1)) | m, j = i + l;
      const int jj = m << k;
      const int wr = T.sin1024[jj + 256], wi = inverse ? T.sin1024[jj] : (int16_t)(-T.sin1024[jj]);
      const int32_t tr = (wr * fr[2 * j] - wi * fr[2 * j + 1] + 1) >> 1;
      const int32_t ti = (wr * fr[2 * j + 1] + wi * fr[2 * j] + 1) >> 1;
      const int32_t qr = (int32_t)fr[2 * i] * 16384, qi = (int32_t)fr[2 * i + 1] * 16384;
      const int sh = inverse ? shift + 14 : 15;
      fr[2 * j] = (int16_t)((qr - tr + round2) >> sh);
      fr[2 * j + 1] = (int16_t)((qi - ti + round2) >> sh);
      fr[2 * i] = (int16_t)((qr + tr + round2) >> sh);
      fr[2 * i + 1] = (int16_t)((qi + ti + round2) >> sh);
    }
    wsync();
  }
  return scale;
}

// WebRtcSpl_Energy over GetScalingSquare: the scaling from the largest |v| (as int16, so -32768 stays
// negative, as there), then a wrapping sum of (v * v) >> scaling.
NSX_HD inline int32_t energy(const int16_t* v, int n, int* scale_out, Lanes L) {
  int32_t smax = -1;
  for (int i = L.id; i < n; i += L.n) {
    const int16_t sabs = (int16_t)(v[i] > 0 ? v[i] : -v[i]);
    smax = sabs > smax ? sabs : smax;
  }
  smax = wmax(smax);
  const int nbits = 32 - norm_u32((uint32_t)n);
  const int t = norm_w32(smax * smax);
  const int scaling = smax == 0 ? 0 : (t > nbits ? 0 : nbits - t);
  uint32_t en = 0;
  for (int i = L.id; i < n; i += L.n) en += (uint32_t)(mul16(v[i], v[i]) >> scaling);
  *scale_out = scaling;
  return (int32_t)wsum(en);
}

// buf[0 .. len) <- buf[bl .. len) ++ src[0 .. bl): through tmp, so that no lane overwrites what another reads
NSX_HD inline void shift_in(int16_t* buf, int len, int bl, const int16_t* src, int16_t* tmp, Lanes L) {
  for (int i = L.id; i < len; i += L.n) tmp[i] = i < len - bl ? buf[i + bl] : (src ? src[i - (len - bl)] : (int16_t)0);
  wsync();
  for (int i = L.id; i < len; i += L.n) buf[i] = tmp[i];
  wsync();
}

// ------------------------------------------------------------------ WebRtcNsx_DataAnalysis
NSX_HD inline void data_analysis(AspNsxState& s, NsxWork& w, const int16_t* speech, const NsxTables& T, Lanes L) {
  const int anaLen = s.anaLen, anaLen2 = s.anaLen2, bl = s.blockLen10ms, stages = s.stages;
  const int16_t* window = anaLen == 128 ? T.win128 : T.win256;
  shift_in(s.analysisBuffer, anaLen, bl, speech, w.win, L);
  int32_t mx = 0;
  for (int i = L.id; i < anaLen; i += L.n) {
    const int16_t v = (int16_t)mul16_rsft_round(window[i], s.analysisBuffer[i], 14);
    w.win[i] = v;
    const int32_t a = v < 0 ? -(int32_t)v : (int32_t)v;
    mx = a > mx ? a : mx;
  }
  wsync();
  int scaleIn;
  const int32_t eIn = energy(w.win, anaLen, &scaleIn, L);
  mx = wmax(mx);
  if (mx > 32767) mx = 32767;
  const int normData = norm_w16(mx);
  const int minNorm0 = s.minNorm, blockIndex = s.blockIndex;
  const int rs_magn0 = normData - minNorm0;
  const int rs_init = rs_magn0 < 0 ? -rs_magn0 : 0;
  const int rs_magn = rs_magn0 > 0 ? rs_magn0 : 0;
  if (L.id == 0) {
    s.energyIn = eIn;
    s.scaleEnergyIn = scaleIn;
    s.zeroInputSignal = mx == 0;
    s.normData = normData;
    if (mx != 0) s.minNorm = minNorm0 - rs_init;
  }
  if (mx == 0) {
    wsync();
    return;
  }
  const int net_norm = stages - normData;
  // NormalizeRealBuffer + RealForwardFFT: (x << normData, 0) straight to its bit-reversed place
  for (int i = L.id; i < anaLen; i += L.n) {
    const int r = bitrev(i, stages);
    w.cb[2 * r] = (int16_t)((uint32_t)(int32_t)w.win[i] << normData);
    w.cb[2 * r + 1] = 0;
  }
  wsync();
  complex_fft(w.cb, stages, false, T, L);
  const bool startup = blockIndex < 50;
  uint32_t e_sum = 0, m_sum = 0, slm = 0, slilm = 0;
  for (int i = L.id; i <= anaLen2; i += L.n) {
    const int16_t re = w.cb[2 * i], im = w.cb[2 * i + 1];
    uint32_t e, m;
    s.real[i] = re;
    if (i == 0 || i == anaLen2) {
      s.imag[i] = 0;
      e = (uint32_t)mul16(re, re);
      m = (uint16_t)(re >= 0 ? re : -re);
    } else {
      s.imag[i] = (int16_t)(-im);
      e = (uint32_t)mul16(re, re) + (uint32_t)mul16(im, im);
      m = (uint16_t)sqrt_floor((int32_t)e);
    }
    w.magn[i] = (uint16_t)m;
    e_sum += e;
    m_sum += m;
    if (startup) {
      s.initMagnEst[i] = (s.initMagnEst[i] >> rs_init) + (m >> rs_magn);
      if (i >= kStartBand) {
        const int l2 = m ? (int16_t)log2_q8(m, T) : 0;
        slm += (uint32_t)l2;
        slilm += (uint32_t)((T.logIndex[i] * l2) >> 3);
      }
    }
  }
  e_sum = wsum(e_sum);
  m_sum = wsum(m_sum);
  if (startup) {
    slm = wsum(slm);
    slilm = wsum(slilm);
  }
  if (L.id == 0) {
    s.magnEnergy = e_sum;
    s.sumMagn = m_sum;
    if (startup) {
      const int32_t sum_log_magn = (int32_t)slm, sum_log_i_log_magn = (int32_t)slilm;
      const int magnLen = anaLen2 + 1;
      uint32_t tmpU = (uint32_t)m_sum * (uint32_t)s.overdrive;
      tmpU >>= stages + 8;
      tmpU >>= rs_magn;
      s.whiteNoiseLevel = (s.whiteNoiseLevel >> rs_init) + tmpU;
      int16_t det = T.detEstMatrix[kStartBand], sum_log_i = T.sumLogIndex[kStartBand],
              sum_log_i_square = T.sumSqLogIndex[kStartBand];
      if (s.fs == 8000) {
        int32_t t1 = det;
        t1 += mul16(T.sumLogIndex[65], sum_log_i) >> 9;
        t1 -= mul16(T.sumLogIndex[65], T.sumLogIndex[65]) >> 10;
        t1 -= (int32_t)sum_log_i_square << 4;
        t1 -= mul16((int16_t)(magnLen - kStartBand), T.sumSqLogIndex[65]) >> 2;
        det = (int16_t)t1;
        sum_log_i = (int16_t)(sum_log_i - T.sumLogIndex[65]);
        sum_log_i_square = (int16_t)(sum_log_i_square - T.sumSqLogIndex[65]);
      }
      int zeros = 16 - norm_w32(sum_log_magn);
      if (zeros < 0) zeros = 0;
      int32_t t1 = (int32_t)((uint32_t)sum_log_magn << 1);
      const uint16_t slm_u16 = (uint16_t)(t1 >> zeros);
      int32_t t2 = (int32_t)sum_log_i_square * (int32_t)slm_u16;
      uint32_t u1 = (uint32_t)(sum_log_i_log_magn >> 12);
      uint16_t tmp_u16 = (uint16_t)((uint16_t)sum_log_i << 1);
      if ((uint32_t)(int32_t)sum_log_i > u1)
        tmp_u16 = (uint16_t)(tmp_u16 >> zeros);
      else
        u1 >>= zeros;
      t2 = wrap_sub(t2, (int32_t)(u1 * (uint32_t)tmp_u16));
      det = (int16_t)(det >> zeros);
      t2 = div_w32w16(t2, det);
      t2 = wrap_add(t2, (int32_t)((uint32_t)net_norm << 11));
      if (t2 < 0) t2 = 0;
      s.pinkNoiseNumerator = wrap_add(s.pinkNoiseNumerator, t2);
      t2 = (int32_t)sum_log_i * (int32_t)slm_u16;
      t1 = sum_log_i_log_magn >> (3 + zeros);
      t1 = wrap_mul(t1, magnLen - kStartBand);
      t2 = wrap_sub(t2, t1);
      if (t2 > 0) {
        t1 = div_w32w16(t2, det);
        s.pinkNoiseExp += t1 > 16384 ? 16384 : t1 < 0 ? 0 : t1;
      }
    }
  }
  wsync();
}

// ------------------------------------------------------------------ WebRtcNsx_ComputeSpectralFlatness
NSX_HD inline void spectral_flatness(AspNsxState& s, const NsxWork& w, const NsxTables& T, Lanes L) {
  uint32_t num = 0, nzero = 0;
  for (int i = L.id; i < s.magnLen; i += L.n) {
    if (i == 0) continue;
    if (w.magn[i])
      num += (uint32_t)log2_q8(w.magn[i], T);
    else
      ++nzero;
  }
  num = wsum(num);
  nzero = wsum(nzero);
  if (L.id == 0) {
    if (nzero) {
      const uint32_t t = s.featureSpecFlat * 4915u;
      s.featureSpecFlat -= t >> 14;
    } else {
      const int stages = s.stages;
      const uint32_t den = s.sumMagn - (uint32_t)w.magn[0];
      int32_t t32 = log2_q8(den, T);
      int32_t lcs = (int32_t)num;
      lcs = wrap_add(lcs, (int32_t)((uint32_t)(stages - 1) << (stages + 7)));
      lcs = wrap_sub(lcs, (int32_t)((uint32_t)t32 << (stages - 1)));
      lcs = (int32_t)((uint32_t)lcs << (10 - stages));
      const int32_t a = lcs < 0 ? (int32_t)(0u - (uint32_t)lcs) : lcs;
      t32 = (int32_t)(0x00020000 | (a & 0x0001FFFF));
      const int16_t intPart = (int16_t)(7 - (lcs >> 17));
      const int32_t cur = intPart > 0 ? t32 >> intPart : (int32_t)((uint32_t)t32 << -intPart);
      t32 = wrap_sub(cur, (int32_t)s.featureSpecFlat);
      t32 = wrap_mul(t32, 4915);
      s.featureSpecFlat += (uint32_t)(t32 >> 14);
    }
  }
  wsync();
}

// ------------------------------------------------------------------ NoiseEstimationC
NSX_HD inline void update_noise_estimate(AspNsxState& s, int offset, Lanes L) {
  const int magnLen = s.magnLen;
  int32_t mxq = -32768;
  for (int i = L.id; i < magnLen; i += L.n) {
    const int32_t v = s.noiseEstLogQuantile[offset + i];
    mxq = v > mxq ? v : mxq;
  }
  mxq = wmax(mxq);
  const int qNoise = 14 - (int)((11819 * mxq + (1 << 20)) >> 21);
  if (L.id == 0) s.qNoise = qNoise;
  for (int i = L.id; i < magnLen; i += L.n) {
    const int32_t t2 = 11819 * s.noiseEstLogQuantile[offset + i];
    int32_t t1 = 0x00200000 | (t2 & 0x001FFFFF);
    int16_t t16 = (int16_t)(t2 >> 21);
    t16 = (int16_t)(t16 - 21);
    t16 = (int16_t)(t16 + (int16_t)qNoise);
    if (t16 < 0)
      t1 = -t16 > 31 ? 0 : t1 >> -t16;
    else
      t1 = (int32_t)((uint32_t)t1 << t16);
    s.noiseEstQuantile[i] = sat_w16(t1);
  }
}

NSX_HD inline int noise_estimation(AspNsxState& s, NsxWork& w, const NsxTables& T, Lanes L) {
  const int magnLen = s.magnLen, blockIndex = s.blockIndex;
  const int tabind = s.stages - s.normData;
  const int16_t logval = (int16_t)(tabind < 0 ? -T.logTable[-tabind] : T.logTable[tabind]);
  for (int i = L.id; i < magnLen; i += L.n) {
    int16_t lm = logval;
    if (w.magn[i]) {
      const int16_t l2 = (int16_t)log2_q8(w.magn[i], T);
      lm = (int16_t)(mul16(l2, 22713) >> 15);
      lm = (int16_t)(lm + logval);
    }
    w.lmagn[i] = lm;
  }
  int offset = 0;
  for (int sm = 0; sm < 3; ++sm) {
    offset = sm * magnLen;
    const int16_t counter = s.noiseEstCounter[sm];
    const int16_t countDiv = T.counterDiv[counter];
    const int16_t countProd = (int16_t)(counter * countDiv);
    for (int i = L.id; i < magnLen; i += L.n) {
      int16_t q = s.noiseEstLogQuantile[offset + i];
      const int16_t dens = s.noiseEstDensity[offset + i];
      int16_t delta;
      if (dens > 512) {
        delta = (int16_t)(2621440 >> (14 - norm_w16(dens)));
      } else {
        delta = blockIndex < 200 ? 1024 : 5120;
      }
      int16_t t16 = (int16_t)(mul16(delta, countDiv) >> 14);
      const int16_t lm = w.lmagn[i];
      if (lm > q) {
        t16 = (int16_t)(t16 + 2);
        q = (int16_t)(q + t16 / 4);
      } else {
        t16 = (int16_t)(t16 + 1);
        const int16_t t2 = (int16_t)(mul16(t16 / 2, 3) >> 1);
        q = (int16_t)(q - t2);
        if (q < logval) q = logval;
      }
      s.noiseEstLogQuantile[offset + i] = q;
      const int d = lm - q;
      if ((d < 0 ? -d : d) < 3) {
        const int16_t a = (int16_t)mul16_rsft_round(dens, countProd, 15);
        const int16_t b = (int16_t)mul16_rsft_round(21845, countDiv, 15);
        s.noiseEstDensity[offset + i] = (int16_t)(a + b);
      }
    }
    wsync();
    int16_t c = counter;
    if (counter >= 200) {
      c = 0;
      if (blockIndex >= 200) update_noise_estimate(s, offset, L);
    }
    if (L.id == 0) s.noiseEstCounter[sm] = (int16_t)(c + 1);
  }
  if (blockIndex < 200) update_noise_estimate(s, offset, L);
  wsync();
  for (int i = L.id; i < magnLen; i += L.n) w.noise[i] = (uint32_t)(int32_t)s.noiseEstQuantile[i];
  return (int16_t)s.qNoise;
}

// WebRtcNsx_CalcParametricNoiseEstimate: leaves the outputs alone when the exponent is not positive
NSX_HD inline void parametric_noise(int minNorm, int stages, int blockIndex, int16_t exp_avg, int32_t num_avg,
                                    int freq_index, uint32_t* est, uint32_t* est_avg, const NsxTables& T) {
  int32_t t2 = (exp_avg * T.logIndex[freq_index]) >> 15;
  int32_t t1 = wrap_sub(num_avg, t2);
  t1 = wrap_add(t1, (int32_t)((uint32_t)(minNorm - stages) << 11));
  if (t1 > 0) {
    const int16_t int_part = (int16_t)(t1 >> 11), frac_part = (int16_t)(t1 & 0x7ff);
    if (frac_part >> 10) {
      t2 = (2048 - frac_part) * 1244;
      t2 = 2048 - (t2 >> 10);
    } else {
      t2 = (frac_part * 804) >> 10;
    }
    t2 = shift_w32(t2, int_part - 11);
    *est_avg = (uint32_t)(int_part < 32 ? 1u << int_part : 0u) + (uint32_t)t2;
    *est = *est_avg * (uint32_t)(blockIndex + 1);
  }
}

// ------------------------------------------------------------------ WebRtcNsx_ComputeSpectralDifference
NSX_HD inline void spectral_difference(AspNsxState& s, const NsxWork& w, Lanes L) {
  const int magnLen = s.magnLen, stages = s.stages;
  uint32_t sum = 0;
  int32_t maxP = 0, minP = s.avgMagnPause[0];
  for (int i = L.id; i < magnLen; i += L.n) {
    const int32_t v = s.avgMagnPause[i];
    sum += (uint32_t)v;
    maxP = v > maxP ? v : maxP;
    minP = v < minP ? v : minP;
  }
  const int32_t avgPause = (int32_t)wsum(sum) >> (stages - 1);
  maxP = wmax(maxP);
  minP = wmin(minP);
  const int32_t avgMagn = (int32_t)(s.sumMagn >> (stages - 1));
  const int32_t a = wrap_sub(maxP, avgPause), b = wrap_sub(avgPause, minP);
  int nShifts = 10 + stages - norm_w32(a > b ? a : b);
  if (nShifts < 0) nShifts = 0;
  uint32_t varMagn = 0, varPause = 0, cov = 0;
  for (int i = L.id; i < magnLen; i += L.n) {
    const int16_t t16 = (int16_t)((int32_t)w.magn[i] - avgMagn);
    const int32_t t2 = wrap_sub(s.avgMagnPause[i], avgPause);
    varMagn += (uint32_t)(t16 * t16);
    cov += (uint32_t)t2 * (uint32_t)(int32_t)t16;
    const int32_t t1 = t2 >> nShifts;
    varPause += (uint32_t)t1 * (uint32_t)t1;
  }
  varMagn = wsum(varMagn);
  varPause = wsum(varPause);
  const int32_t covS = (int32_t)wsum(cov);
  if (L.id == 0) {
    const int normData = s.normData;
    s.curAvgMagnEnergy += s.magnEnergy >> (2 * normData + stages - 1);
    uint32_t avgDiff = varMagn;
    if (varPause && covS) {
      uint32_t u1 = covS < 0 ? 0u - (uint32_t)covS : (uint32_t)covS;
      const int norm32 = norm_u32(u1) - 16;
      if (norm32 > 0)
        u1 <<= norm32;
      else
        u1 >>= -norm32;
      const uint32_t u2 = u1 * u1;
      nShifts += norm32;
      nShifts <<= 1;
      if (nShifts < 0) {
        varPause = -nShifts > 31 ? 0 : varPause >> (-nShifts);
        nShifts = 0;
      }
      if (varPause > 0) {
        u1 = u2 / varPause;
        u1 = nShifts > 31 ? 0 : u1 >> nShifts;
        avgDiff -= avgDiff < u1 ? avgDiff : u1;
      } else {
        avgDiff = 0;
      }
    }
    const uint32_t u1 = avgDiff >> (2 * normData);
    if (s.featureSpecDiff > u1) {
      const uint32_t u2 = (s.featureSpecDiff - u1) * 77u;
      s.featureSpecDiff -= u2 >> 8;
    } else {
      const uint32_t u2 = (u1 - s.featureSpecDiff) * 77u;
      s.featureSpecDiff += u2 >> 8;
    }
  }
  wsync();
}

// ------------------------------------------------------------------ WebRtcNsx_FeatureParameterExtraction
// (one lane: three histogram increments per frame; the peak search once per 512 frames)
NSX_HD inline void two_peaks(const int16_t* h, uint32_t* pos1, uint32_t* pos2, int* w1, int* w2) {
  int maxPeak1 = 0, maxPeak2 = 0;
  *pos1 = *pos2 = 0;
  *w1 = *w2 = 0;
  for (int i = 0; i < kHist; ++i) {
    if (h[i] > maxPeak1) {
      maxPeak2 = maxPeak1;
      *w2 = *w1;
      *pos2 = *pos1;
      maxPeak1 = h[i];
      *w1 = h[i];
      *pos1 = (uint32_t)(2 * i + 1);
    } else if (h[i] > maxPeak2) {
      maxPeak2 = h[i];
      *w2 = h[i];
      *pos2 = (uint32_t)(2 * i + 1);
    }
  }
}
NSX_HD inline void feature_parameter_extraction(AspNsxState& s, int16_t* histLrt, int16_t* histFlat, int16_t* histDiff,
                                                int flag) {
  if (!flag) {
    uint32_t hi = (uint32_t)s.featureLogLrt;
    if (hi < (uint32_t)kHist) histLrt[hi]++;
    hi = (s.featureSpecFlat * 5) >> 8;
    if (hi < (uint32_t)kHist) histFlat[hi]++;
    hi = kHist;
    if (s.timeAvgMagnEnergy > 0) hi = ((s.featureSpecDiff * 5) >> s.stages) / s.timeAvgMagnEnergy;
    if (hi < (uint32_t)kHist) histDiff[hi]++;
    return;
  }
  int useDiff = 1;
  int32_t avgHist = 0, avgSq = 0;
  int16_t num = 0;
  int i;
  for (i = 0; i < 10; ++i) {
    const int16_t j = (int16_t)(2 * i + 1);
    const int32_t t = histLrt[i] * j;
    avgHist = wrap_add(avgHist, t);
    num = (int16_t)(num + histLrt[i]);
    avgSq = wrap_add(avgSq, wrap_mul(t, j));
  }
  int32_t avgCompl = avgHist;
  for (; i < kHist; ++i) {
    const int16_t j = (int16_t)(2 * i + 1);
    const int32_t t = histLrt[i] * j;
    avgCompl = wrap_add(avgCompl, t);
    avgSq = wrap_add(avgSq, wrap_mul(t, j));
  }
  const int32_t fluct = wrap_sub(wrap_mul(avgSq, num), wrap_mul(avgHist, avgCompl));
  const int32_t thresFluct = 10240 * num;
  const uint32_t tmpU = 6u * (uint32_t)avgHist;
  if (fluct < thresFluct || num == 0 || tmpU > (uint32_t)(100 * num)) {
    s.thresholdLogLrt = s.maxLrt;
  } else {
    const int32_t t = (int32_t)((tmpU << (9 + s.stages)) / (uint32_t)(int32_t)num / 25);
    s.thresholdLogLrt = t > s.maxLrt ? s.maxLrt : t < s.minLrt ? s.minLrt : t;
  }
  if (fluct < thresFluct) useDiff = 0;
  uint32_t p1, p2;
  int w1, w2;
  two_peaks(histFlat, &p1, &p2, &w1, &w2);
  int useFlat = 1;
  if (p1 - p2 < 4 && w2 * 2 > w1) {
    w1 += w2;
    p1 = (p1 + p2) >> 1;
  }
  if (w1 < 154 || p1 < 24) {
    useFlat = 0;
  } else {
    const uint32_t v = 922u * p1;
    s.thresholdSpecFlat = v > 38912u ? 38912u : v < 4096u ? 4096u : v;
  }
  if (useDiff) {
    two_peaks(histDiff, &p1, &p2, &w1, &w2);
    if (p1 - p2 < 4 && w2 * 2 > w1) {
      w1 += w2;
      p1 = (p1 + p2) >> 1;
    }
    const uint32_t v = 6u * p1;
    s.thresholdSpecDiff = v > 100u ? 100u : v < 16u ? 16u : v;
    if (w1 < 154) useDiff = 0;
  }
  const int featureSum = 6 / (1 + useFlat + useDiff);
  s.weightLogLrt = (int16_t)featureSum;
  s.weightSpecFlat = (int16_t)(useFlat * featureSum);
  s.weightSpecDiff = (int16_t)(useDiff * featureSum);
  for (i = 0; i < kHist; ++i) histLrt[i] = histDiff[i] = histFlat[i] = 0;
}

// kIndicatorTable lookup with linear interpolation, shared by the three features
NSX_HD inline int16_t indicator(uint32_t x14, bool above, bool round, const NsxTables& T) {
  int16_t ind = above ? 16384 : 0;
  const int16_t tableIndex = (int16_t)(x14 >> 14);
  if (tableIndex < 16 && tableIndex >= 0) {
    int16_t t2 = T.indicator[tableIndex];
    const int16_t t1 = (int16_t)(T.indicator[tableIndex + 1] - T.indicator[tableIndex]);
    const int16_t frac = (int16_t)(x14 & 0x3fff);
    t2 = (int16_t)(t2 + (int16_t)(round ? mul16_rsft_round(t1, frac, 14) : mul16(t1, frac) >> 14));
    ind = (int16_t)(above ? 8192 + t2 : 8192 - t2);
  }
  return ind;
}

// ------------------------------------------------------------------ WebRtcNsx_SpeechNoiseProb
NSX_HD inline void speech_noise_prob(AspNsxState& s, NsxWork& w, const NsxTables& T, Lanes L) {
  const int magnLen = s.magnLen, stages = s.stages;
  uint32_t ksum = 0;
  for (int i = L.id; i < magnLen; i += L.n) {
    const uint32_t post = w.postSnr[i], prior = w.priorSnr[i];
    int32_t bessel = (int32_t)post;
    const int normTmp = norm_u32(post);
    const uint32_t num = post << normTmp;
    const uint32_t den = normTmp > 10 ? prior << (normTmp - 11) : prior >> (11 - normTmp);
    if (den > 0)
      bessel = wrap_sub(bessel, (int32_t)(num / den));
    else
      bessel = 0;
    const uint32_t zeros = (uint32_t)norm_u32(prior);
    int32_t frac32 = (int32_t)(((prior << zeros) & 0x7FFFFFFF) >> 19);
    int32_t t32 = (frac32 * frac32 * -43) >> 19;
    t32 += mul16((int16_t)frac32, 5412) >> 12;
    frac32 = t32 + 37;
    t32 = (int32_t)(((31 - zeros) << 12) + (uint32_t)frac32) - (11 << 12);
    const int32_t logTmp = wrap_mul(t32, 178) >> 8;
    const int32_t t1 = wrap_add(logTmp, s.logLrtTimeAvgW32[i]) / 2;
    const int32_t v = wrap_add(s.logLrtTimeAvgW32[i], wrap_sub(bessel, t1));
    s.logLrtTimeAvgW32[i] = v;
    ksum += (uint32_t)v;
  }
  const int32_t ksumS = (int32_t)wsum(ksum);
  if (L.id == 0) {
    s.featureLogLrt = wrap_mul(ksumS, 10) >> (stages + 11);
    int32_t t1 = wrap_sub(ksumS, s.thresholdLogLrt);
    int nShifts = 7 - stages;
    bool above = true;
    if (t1 < 0) {
      above = false;
      t1 = (int32_t)(0u - (uint32_t)t1);
      nShifts++;
    }
    t1 = shift_w32(t1, nShifts);
    int32_t indPrior = s.weightLogLrt * indicator((uint32_t)t1, above, false, T);
    if (s.weightSpecFlat) {
      const uint32_t u1 = s.featureSpecFlat * 400u;
      uint32_t u2 = s.thresholdSpecFlat - u1;
      nShifts = 4;
      above = true;
      if (s.thresholdSpecFlat < u1) {
        above = false;
        u2 = u1 - s.thresholdSpecFlat;
        nShifts++;
      }
      const uint32_t x = div_u32u16(u2 << nShifts, 25);
      // the reference tests tableIndex < 16 only: a negative int16 index reads in front of its table;
      // x >> 14 stays below 2^15 for every reachable feature value (featureSpecFlat is Q10, < 2^20)
      indPrior += s.weightSpecFlat * indicator(x, above, false, T);
    }
    if (s.weightSpecDiff) {
      uint32_t u1 = 0;
      if (s.featureSpecDiff) {
        const int nz = norm_u32(s.featureSpecDiff);
        const int normTmp = 20 - stages < nz ? 20 - stages : nz;
        u1 = s.featureSpecDiff << normTmp;
        const uint32_t u2 = s.timeAvgMagnEnergy >> (20 - stages - normTmp);
        u1 = u2 > 0 ? u1 / u2 : 0x7fffffffu;
      }
      const uint32_t u3 = (s.thresholdSpecDiff << 17) / 25;
      uint32_t u2 = u1 - u3;
      nShifts = 1;
      above = true;
      if (u2 & 0x80000000u) {
        above = false;
        u2 = u3 - u1;
        nShifts--;
      }
      indPrior += s.weightSpecDiff * indicator(u2 >> nShifts, above, true, T);
    }
    const int16_t indPrior16 = (int16_t)((98307 - indPrior) / 6);
    const int16_t t16 = (int16_t)(indPrior16 - s.priorNonSpeechProb);
    s.priorNonSpeechProb = (int16_t)(s.priorNonSpeechProb + (int16_t)(mul16(1638, t16) >> 14));
  }
  wsync();
  const int32_t prior = s.priorNonSpeechProb;
  for (int i = L.id; i < magnLen; i += L.n) {
    uint16_t nsp = 0;
    const int32_t lrt = s.logLrtTimeAvgW32[i];
    if (prior > 0 && lrt < 65300) {
      int32_t t1 = wrap_mul(lrt, 23637) >> 14;
      int16_t intPart = (int16_t)(t1 >> 12);
      if (intPart < -8) intPart = -8;
      const int16_t frac = (int16_t)(t1 & 0xfff);
      int32_t t2 = (frac * frac * 44) >> 19;
      t2 += mul16(frac, 84) >> 7;
      int32_t invLrt = (int32_t)(1u << (8 + intPart)) + shift_w32(t2, intPart - 4);
      const int normTmp = norm_w32(invLrt), normTmp2 = norm_w16((int16_t)(16384 - prior));
      if (normTmp + normTmp2 >= 7) {
        if (normTmp + normTmp2 < 15) {
          invLrt >>= 15 - normTmp2 - normTmp;
          t1 = wrap_mul(invLrt, 16384 - prior);
          invLrt = shift_w32(t1, 7 - normTmp - normTmp2);
        } else {
          t1 = wrap_mul(invLrt, 16384 - prior);
          invLrt = t1 >> 8;
        }
        t1 = prior << 8;
        const int32_t d = wrap_add(prior, invLrt);
        nsp = d != 0 ? (uint16_t)(t1 / d) : (uint16_t)0;
      }
    }
    w.nsp[i] = nsp;
  }
  wsync();
}

// ------------------------------------------------------------------ WebRtcNsx_DataSynthesis
NSX_HD inline void data_synthesis(AspNsxState& s, NsxWork& w, int16_t* out, const NsxTables& T, Lanes L) {
  const int anaLen = s.anaLen, anaLen2 = s.anaLen2, bl = s.blockLen10ms, stages = s.stages;
  if (s.zeroInputSignal) {
    for (int i = L.id; i < bl; i += L.n) out[i] = s.synthesisBuffer[i];
    wsync();
    shift_in(s.synthesisBuffer, anaLen, bl, nullptr, w.win, L);
    return;
  }
  // PrepareSpectrum
  for (int i = L.id; i <= anaLen2; i += L.n) {
    s.real[i] = (int16_t)(mul16(s.real[i], (int16_t)s.noiseSupFilter[i]) >> 14);
    s.imag[i] = (int16_t)(mul16(s.imag[i], (int16_t)s.noiseSupFilter[i]) >> 14);
  }
  wsync();
  // RealInverseFFT: the conjugate-symmetric spectrum straight to its bit-reversed place
  for (int k = L.id; k < anaLen; k += L.n) {
    const int r = bitrev(k, stages);
    if (k <= anaLen2) {
      w.cb[2 * r] = s.real[k];
      w.cb[2 * r + 1] = (int16_t)(-s.imag[k]);
    } else {
      w.cb[2 * r] = s.real[anaLen - k];
      w.cb[2 * r + 1] = (int16_t)(-(int16_t)(-s.imag[anaLen - k]));
    }
  }
  wsync();
  const int outCIFFT = complex_fft(w.cb, stages, true, T, L);
  // Denormalize
  const int normData = s.normData;
  for (int i = L.id; i < anaLen; i += L.n) s.real[i] = sat_w16(shift_w32((int32_t)w.cb[2 * i], outCIFFT - normData));
  wsync();
  int16_t gainFactor = 8192;
  if (s.gainMap == 1 && s.blockIndex > 200 && s.energyIn > 0) {
    int scaleOut = 0;
    int32_t energyOut = energy(s.real, anaLen, &scaleOut, L);
    int32_t energyIn = s.energyIn;
    if (scaleOut == 0 && !(energyOut & 0x7f800000))
      energyOut = shift_w32(energyOut, 8 + scaleOut - s.scaleEnergyIn);
    else
      energyIn >>= 8 + scaleOut - s.scaleEnergyIn;
    if (L.id == 0) s.energyIn = energyIn;
    // the reference asserts energyIn > 0 here; a ratio of 0 stands in where it would have stopped
    int16_t ratio = energyIn > 0 ? (int16_t)(wrap_add(energyOut, energyIn / 2) / energyIn) : (int16_t)0;
    ratio = ratio > 256 ? 256 : ratio < 0 ? 0 : ratio;
    const int16_t g1 = T.factor1[ratio], g2 = T.factor2[s.aggrMode - 1][ratio];
    const int16_t a = (int16_t)(mul16(16384 - s.priorNonSpeechProb, g1) >> 14);
    const int16_t b = (int16_t)(mul16(s.priorNonSpeechProb, g2) >> 14);
    gainFactor = (int16_t)(a + b);
  }
  // SynthesisUpdate
  const int16_t* window = anaLen == 128 ? T.win128 : T.win256;
  for (int i = L.id; i < anaLen; i += L.n) {
    const int16_t a = (int16_t)mul16_rsft_round(window[i], s.real[i], 14);
    const int32_t t = mul16_rsft_round(a, gainFactor, 13);
    const int16_t v = add_sat_w16(s.synthesisBuffer[i], sat_w16(t));
    s.synthesisBuffer[i] = v;
    if (i < bl) out[i] = v;
  }
  wsync();
  shift_in(s.synthesisBuffer, anaLen, bl, nullptr, w.win, L);
}

// ------------------------------------------------------------------ WebRtcNsx_ProcessCore
// in / out: num_bands pointers to blockLen10ms samples; hist: the stream's three histograms
NSX_HD inline void process_core(AspNsxState& s, NsxWork& w, int16_t* hist, const int16_t* const* in, int num_bands,
                                int16_t* const* out, const NsxTables& T, Lanes L) {
  const int anaLen = s.anaLen, anaLen2 = s.anaLen2, magnLen = s.magnLen, bl = s.blockLen10ms, stages = s.stages;
  data_analysis(s, w, in[0], T, L);
  if (s.zeroInputSignal) {
    data_synthesis(s, w, out[0], T, L);
    for (int b = 1; b < num_bands; ++b) {
      shift_in(s.dataBufHBFX[b - 1], anaLen, bl, in[b], w.win, L);
      for (int j = L.id; j < bl; j += L.n) out[b][j] = s.dataBufHBFX[b - 1][j];
    }
    wsync();
    return;
  }
  const int blockIndex = s.blockIndex + 1;
  wsync();
  if (L.id == 0) s.blockIndex = blockIndex;
  wsync();
  const int normData = s.normData;
  const int16_t qMagn = (int16_t)(normData - stages);
  spectral_flatness(s, w, T, L);
  int16_t qNoise = (int16_t)noise_estimation(s, w, T, L);
  for (int i = L.id; i < magnLen; i += L.n) w.prevNoiseU16[i] = (uint16_t)(s.prevNoiseU32[i] >> 11);
  const uint16_t overdrive = s.overdrive, denoiseBound = s.denoiseBound;
  if (blockIndex < 50) {
    const int minNorm = s.minNorm;
    const int q_dom = qNoise < minNorm - stages ? qNoise : minNorm - stages;
    const int32_t pinkExp = s.pinkNoiseExp;
    int16_t exp_avg = 0;
    int32_t num_avg = 0;
    uint32_t est0 = 0, est_avg0 = 0;
    if (pinkExp) {
      exp_avg = (int16_t)div_w32w16(pinkExp, (int16_t)(blockIndex + 1));
      num_avg = div_w32w16(s.pinkNoiseNumerator, (int16_t)(blockIndex + 1));
      parametric_noise(minNorm, stages, blockIndex, exp_avg, num_avg, kStartBand, &est0, &est_avg0, T);
    } else {
      est0 = s.whiteNoiseLevel;
      est_avg0 = est0 / (uint32_t)(blockIndex + 1);
    }
    for (int i = L.id; i < magnLen; i += L.n) {
      uint32_t est = est0, est_avg = est_avg0;
      if (pinkExp && i >= kStartBand) {
        est = est_avg = 0;
        parametric_noise(minNorm, stages, blockIndex, exp_avg, num_avg, i, &est, &est_avg, T);
      }
      uint16_t ft = denoiseBound;
      const uint32_t ime = s.initMagnEst[i];
      if (ime) {
        uint32_t u1 = est * (uint32_t)overdrive;
        uint32_t numer = ime << 8;
        if (numer > u1) {
          numer -= u1;
          int ns = norm_u32(numer);
          ns = ns > 6 ? 6 : ns;
          numer <<= ns;
          u1 = ime >> (6 - ns);
          if (u1 == 0) u1 = 1;
          const uint32_t u2 = numer / u1;
          ft = (uint16_t)(u2 > 16384u ? 16384u : u2 < (uint32_t)denoiseBound ? (uint32_t)denoiseBound : u2);
        }
      }
      w.filtTmp[i] = ft;
      uint32_t u1 = w.noise[i] >> (qNoise - q_dom);
      uint32_t u2 = est_avg >> (minNorm - stages - q_dom);
      int ns = 0;
      if (u1 & 0xfc000000u) {
        u1 >>= 6;
        u2 >>= 6;
        ns = 6;
      }
      u1 *= (uint32_t)blockIndex;
      u2 *= (uint32_t)(50 - blockIndex);
      w.noise[i] = div_u32u16(u1 + u2, 50) << ns;
    }
    qNoise = (int16_t)q_dom;
  }
  if (blockIndex < 200 && L.id == 0) {
    s.timeAvgMagnEnergyTmp += s.magnEnergy >> (2 * normData + stages - 1);
    s.timeAvgMagnEnergy = div_u32u16(s.timeAvgMagnEnergyTmp, (uint16_t)(blockIndex + 1));
  }
  const uint32_t satMax = 1048575u;
  const int prevQMagn = s.prevQMagn, prevQNoise = s.prevQNoise;
  {
    const int postShifts = 6 + qMagn - qNoise;
    const int nShifts = 5 - prevQMagn + prevQNoise;
    for (int i = L.id; i < magnLen; i += L.n) {
      uint32_t post = 2048;
      uint32_t u1 = (uint32_t)w.magn[i] << 6;
      const uint32_t u2 = postShifts < 0 ? w.noise[i] >> -postShifts : w.noise[i] << postShifts;
      if (u1 > u2) {
        u1 <<= 11;
        if (u2 > 0) {
          u1 /= u2;
          post = satMax < u1 ? satMax : u1;
        } else {
          post = satMax;
        }
      }
      w.postSnr[i] = post;
      const uint32_t nearMagnEst = (uint32_t)s.prevMagnU16[i] * (uint32_t)s.noiseSupFilter[i];
      u1 = nearMagnEst << 3;
      const uint32_t p = s.prevNoiseU32[i] >> (nShifts & 31);   // a negative count as the reference build takes it: modulo 32
      if (p > 0) {
        u1 /= p;
        u1 = satMax < u1 ? satMax : u1;
      } else {
        u1 = satMax;
      }
      w.prevNearSnr[i] = u1;
      const uint32_t priorSnr = u1 * 2007u + (post - 2048u) * 41u + 512u;
      w.priorSnr[i] = 2048u + (priorSnr >> 10);
    }
  }
  wsync();
  spectral_difference(s, w, L);
  if (L.id == 0) {
    s.cntThresUpdate++;
    const int flag = s.cntThresUpdate == s.modelUpdate;
    feature_parameter_extraction(s, hist, hist + kHist, hist + 2 * kHist, flag);
    if (flag) {
      s.cntThresUpdate = 0;
      s.curAvgMagnEnergy >>= 9;
      const uint32_t u1 = (s.curAvgMagnEnergy + s.timeAvgMagnEnergy + 1) >> 1;
      if (u1 != s.timeAvgMagnEnergy && s.featureSpecDiff && s.timeAvgMagnEnergy > 0) {
        int norm32 = 0;
        uint32_t u3 = u1;
        while (0xFFFF0000u & u3) {
          u3 >>= 1;
          norm32++;
        }
        uint32_t u2 = s.featureSpecDiff;
        while (0xFFFF0000u & u2) {
          u2 >>= 1;
          norm32++;
        }
        u3 = u3 * u2;
        u3 /= s.timeAvgMagnEnergy;
        if (norm_u32(u3) < norm32) {
          s.featureSpecDiff = 0x007FFFFF;
        } else {
          const uint32_t v = u3 << norm32;
          s.featureSpecDiff = v > 0x007FFFFFu ? 0x007FFFFFu : v;
        }
      }
      s.timeAvgMagnEnergy = u1;
      s.curAvgMagnEnergy = 0;
    }
  }
  wsync();
  speech_noise_prob(s, w, T, L);
  // noise update: bin i starts from the gamma that bin i - 1 left (a function of its probability alone)
  uint32_t maxNoise = 0;
  {
    const int postShifts = prevQNoise - qMagn;
    const int nShifts = prevQMagn - qMagn;
    for (int i = L.id; i < magnLen; i += L.n) {
      uint16_t gammaNoise = (i == 0 || w.nsp[i - 1] >= 205) ? 26 : 3;
      const uint32_t magn = w.magn[i];
      uint32_t u2 = postShifts < 0 ? magn >> -postShifts : magn << postShifts;
      uint32_t u1;
      int sign;
      if (w.prevNoiseU16[i] > u2) {
        sign = -1;
        u1 = w.prevNoiseU16[i] - u2;
      } else {
        sign = 1;
        u1 = u2 - w.prevNoiseU16[i];
      }
      const uint32_t prevNoise = s.prevNoiseU32[i];
      uint32_t upd = prevNoise, u3 = 0;
      const uint16_t nsp = w.nsp[i];
      if (u1 && nsp) {
        u3 = u1 * (uint32_t)nsp;
        u2 = (0x7c000000u & u3) ? (u3 >> 5) * gammaNoise : (u3 * gammaNoise) >> 5;
        upd = sign > 0 ? upd + u2 : upd - u2;
      }
      const uint16_t prevGamma = gammaNoise;
      gammaNoise = nsp < 205 ? 3 : 26;
      if (prevGamma != gammaNoise) {
        u2 = (0x7c000000u & u3) ? (u3 >> 5) * gammaNoise : (u3 * gammaNoise) >> 5;
        u1 = sign > 0 ? prevNoise + u2 : prevNoise - u2;
        if (upd > u1) upd = u1;
      }
      w.noise[i] = upd;
      if (upd > maxNoise) maxNoise = upd;
      int32_t t2 = shift_w32(s.avgMagnPause[i], -nShifts);
      if (nsp > 205) {
        int32_t t1;
        if (nShifts < 0) {
          t1 = wrap_sub((int32_t)magn, t2);
          t1 = wrap_mul(t1, 13);
          t1 = wrap_add(t1, 128) >> 8;
        } else {
          t1 = wrap_sub((int32_t)(magn << nShifts), s.avgMagnPause[i]);
          t1 = wrap_mul(t1, 13);
          t1 = wrap_add(t1, (int32_t)(128u << nShifts)) >> (8 + nShifts);
        }
        t2 = wrap_add(t2, t1);
      }
      s.avgMagnPause[i] = t2;
    }
  }
  maxNoise = wmaxu(maxNoise);
  const int norm32no1 = norm_u32(maxNoise);
  qNoise = (int16_t)(prevQNoise + norm32no1 - 5);
  {
    const int nShifts = prevQNoise + 11 - qMagn;
    for (int i = L.id; i < magnLen; i += L.n) {
      uint32_t cur = 0, tmpMagn, tmpNoise;
      const uint32_t magn = w.magn[i], noise = w.noise[i];
      if (nShifts < 0) {
        tmpMagn = magn;
        tmpNoise = noise << -nShifts;
      } else if (nShifts > 17) {
        tmpMagn = magn << 17;
        tmpNoise = nShifts - 17 > 31 ? 0 : noise >> (nShifts - 17);
      } else {
        tmpMagn = magn << nShifts;
        tmpNoise = noise;
      }
      if (tmpMagn > tmpNoise) {
        uint32_t u1 = tmpMagn - tmpNoise;
        const int nz = norm_u32(u1);
        const int n2 = nz < 11 ? nz : 11;
        u1 <<= n2;
        const uint32_t u2 = tmpNoise >> (11 - n2);
        if (u2 > 0) u1 /= u2;
        cur = satMax < u1 ? satMax : u1;
      }
      const uint32_t priorSnr = w.prevNearSnr[i] * 2007u + cur * 41u;
      const uint32_t u1 = (uint32_t)overdrive + ((priorSnr + 8192u) >> 14);
      const uint16_t t16 = (uint16_t)((priorSnr + u1 / 2) / u1);
      uint16_t filt = t16 > 16384 ? 16384 : t16 < denoiseBound ? denoiseBound : t16;
      if (blockIndex < 50) {
        const uint32_t a = (uint32_t)filt * (uint32_t)blockIndex + (uint32_t)w.filtTmp[i] * (uint32_t)(50 - blockIndex);
        filt = (uint16_t)div_u32u16(a, 50);
      }
      s.noiseSupFilter[i] = filt;
      s.prevNoiseU32[i] = norm32no1 > 5 ? noise << (norm32no1 - 5) : noise >> (5 - norm32no1);
      s.prevMagnU16[i] = (uint16_t)magn;
    }
  }
  if (L.id == 0) {
    s.prevQNoise = qNoise;
    s.prevQMagn = qMagn;
  }
  wsync();
  data_synthesis(s, w, out[0], T, L);
  if (num_bands > 1) {
    uint32_t pSum = 0, fSum = 0;
    for (int i = anaLen2 - (anaLen2 >> 2) + L.id; i < anaLen2; i += L.n) {
      pSum += w.nsp[i];
      fSum += s.noiseSupFilter[i];
    }
    const uint16_t p16 = (uint16_t)wsum(pSum);
    fSum = wsum(fSum);
    const int16_t avgProbSpeechHB = (int16_t)(4096 - (p16 >> (stages - 7)));
    const int16_t avgFilterGainHB = (int16_t)(fSum >> (stages - 3));
    const int16_t gainModHB = avgProbSpeechHB < 3607 ? avgProbSpeechHB : 3607;
    int16_t gainHB;
    if (avgProbSpeechHB < 2048) {
      gainHB = (int16_t)((gainModHB << 1) + (avgFilterGainHB >> 1));
    } else {
      gainHB = (int16_t)(mul16(3, avgFilterGainHB) >> 2);
      gainHB = (int16_t)(gainHB + gainModHB);
    }
    gainHB = gainHB > 16384 ? 16384 : gainHB < (int16_t)denoiseBound ? (int16_t)denoiseBound : gainHB;
    for (int b = 1; b < num_bands; ++b) {
      shift_in(s.dataBufHBFX[b - 1], anaLen, bl, in[b], w.win, L);
      for (int j = L.id; j < bl; j += L.n) out[b][j] = (int16_t)(mul16(gainHB, s.dataBufHBFX[b - 1][j]) >> 14);
    }
    wsync();
  }
}

}  // namespace aspnsx
#endif  // ASP_NSX_CORE_H_
