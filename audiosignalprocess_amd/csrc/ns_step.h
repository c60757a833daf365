// ns_step.h -- the text of the NS frame step that does not depend on how bins sit on lanes, shared by the three
// frame kernels (ns_kernels.hip, ns_kernels1.hip, ns_kernels2.hip): the reference's constants, a quantile tracker's
// step, the histogram-window close, and the step's wave-uniform scalar sections, each a function with its inputs and
// results stated.  The arithmetic forms they use (exact divisions, lean libm) are in ns_device.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ns_device.h"
#include "ns_layout.h"

namespace aspns_dev {
using namespace aspns;

// ns/defines.h:19-48, same (float)<double literal> spelling as the reference
#define NS_QUANTILE (float)0.25
#define NS_END_STARTUP_LONG 200
#define NS_END_STARTUP_SHORT 50
#define NS_FACTOR (float)40.0
#define NS_WIDTH (float)0.01
#define NS_DD_PR_SNR (float)0.98
#define NS_LRT_TAVG (float)0.50
#define NS_SPECT_FL_TAVG (float)0.30
#define NS_SPECT_DIFF_TAVG (float)0.30
#define NS_PRIOR_UPDATE (float)0.10
#define NS_NOISE_UPDATE (float)0.90
#define NS_SPEECH_UPDATE (float)0.99
#define NS_WIDTH_PR_MAP (float)4.0
#define NS_PROB_RANGE (float)0.20
#define NS_GAMMA_PAUSE (float)0.05
#define NS_B_LIM (float)0.5
#define NS_START_BAND 5

// x / NB for the NB bins of a geometry (129; 8 kHz: 65), correctly rounded, the divisor a constant
template <int NB>
__device__ __forceinline__ float ns_div_bins(float a) {
  return div_by_uniform(a, (float)NB, 1.0f / (float)NB);
}
#define DIV129(a) ns_div_bins<kBins>(a)
template <int NB>
__device__ __forceinline__ f32x2 ns_div_bins2(f32x2 a) {  // two at a time (ns_kernels1.hip)
  return div_by_uniform2(a, (float)NB, 1.0f / (float)NB);
}
#define DIV129_2(a) ns_div_bins2<kBins>(a)

// One step of a quantile tracker (ns_core.c:232-260) in the branch-free form of the frame kernels: delta = FACTOR /
// max(density, 1) (the quotient by 1 is exact), the step carries its sign -- lq += (+QUANTILE delta) / n or (-(1 -
// QUANTILE) delta) / n (products, quotients and x + (-y) are sign-symmetric) -- and the density moves where the new
// lq lies within WIDTH of the log magnitude.  cnt = n - 1, cnt1 = n, rcnt1 = 1 / n (rounded) as floats.
// The packed form serves a lane's two owned bins of ONE tracker (cnt, cnt1, rcnt1 wave-uniform); the scalar form
// serves bin 128 of the three trackers at once, tracker s on its own lane with its own cnt / cnt1 / rcnt1: the same
// IEEE operations on the same operands in the same order as three wave-uniform passes.
__device__ __forceinline__ void tracker_step2(f32x2& lq, f32x2& den, f32x2 lm, float cnt, float cnt1, float rcnt1) {
  const f32x2 dm = {fmax_raw(den.x, 1.0f), fmax_raw(den.y, 1.0f)};
  const float fac = NS_FACTOR * 1.f, qp = NS_QUANTILE, qm = -(1.f - NS_QUANTILE), wd = NS_WIDTH;
  const f32x2 delta = fdiv2(f32x2{fac, fac}, dm);
  const f32x2 coef = {lm.x > lq.x ? qp : qm, lm.y > lq.y ? qp : qm};
  const f32x2 rd = {rcnt1, rcnt1}, nd1 = {-cnt1, -cnt1};
  {
    const f32x2 a = coef * delta, q0 = a * rd;
    lq = lq + __builtin_elementwise_fma(__builtin_elementwise_fma(nd1, q0, a), rd, q0);
  }
  const f32x2 a = f32x2{cnt, cnt} * den + f32x2{1.f / (2.f * wd), 1.f / (2.f * wd)}, q0 = a * rd;
  const f32x2 nd = __builtin_elementwise_fma(__builtin_elementwise_fma(nd1, q0, a), rd, q0);
  den = f32x2{fabsf(lm.x - lq.x) < wd ? nd.x : den.x, fabsf(lm.y - lq.y) < wd ? nd.y : den.y};
}
__device__ __forceinline__ void tracker_step1(float& lq, float& den, float lm, float cnt, float cnt1, float rcnt1) {
  const float fac = NS_FACTOR * 1.f, qp = NS_QUANTILE, qm = -(1.f - NS_QUANTILE), wd = NS_WIDTH;
  const float delta = fdiv(fac, fmax_raw(den, 1.0f));
  const float coef = lm > lq ? qp : qm;
  lq = lq + div_by_uniform(coef * delta, cnt1, rcnt1);
  const float nd = div_by_uniform(cnt * den + 1.f / (2.f * wd), cnt1, rcnt1);
  den = fabsf(lm - lq) < wd ? nd : den;
}
// The same two steps with the step quotient in its short form (ns_kernels1.hip; the forms above keep their text).  The
// numerator is the constant FACTOR and the divisor is at least 1, so delta is a function of one float: fdiv_c equals
// fdiv there on every bit pattern max(density, 1) can be (ns_device.h; swept on the device, NaN and +inf included).
__device__ __forceinline__ float fdiv40(float dm) { return fdiv_c(NS_FACTOR * 1.f, dm); }      // dm == max(den, 1)
__device__ __forceinline__ f32x2 fdiv40_2(f32x2 dm) { return fdiv2_c(NS_FACTOR * 1.f, dm); }
__device__ __forceinline__ void tracker_step2_c(f32x2& lq, f32x2& den, f32x2 lm, float cnt, float cnt1, float rcnt1) {
  const f32x2 dm = {fmax_raw(den.x, 1.0f), fmax_raw(den.y, 1.0f)};
  const float qp = NS_QUANTILE, qm = -(1.f - NS_QUANTILE), wd = NS_WIDTH;
  const f32x2 delta = fdiv40_2(dm);
  const f32x2 coef = {lm.x > lq.x ? qp : qm, lm.y > lq.y ? qp : qm};
  lq = lq + div_by_uniform2(coef * delta, cnt1, rcnt1);
  const f32x2 nd = div_by_uniform2(f32x2{cnt, cnt} * den + f32x2{1.f / (2.f * wd), 1.f / (2.f * wd)}, cnt1, rcnt1);
  den = f32x2{fabsf(lm.x - lq.x) < wd ? nd.x : den.x, fabsf(lm.y - lq.y) < wd ? nd.y : den.y};
}
__device__ __forceinline__ void tracker_step1_c(float& lq, float& den, float lm, float cnt, float cnt1, float rcnt1) {
  const float qp = NS_QUANTILE, qm = -(1.f - NS_QUANTILE), wd = NS_WIDTH;
  const float delta = fdiv40(fmax_raw(den, 1.0f));
  const float coef = lm > lq ? qp : qm;
  lq = lq + div_by_uniform(coef * delta, cnt1, rcnt1);
  const float nd = div_by_uniform(cnt * den + 1.f / (2.f * wd), cnt1, rcnt1);
  den = fabsf(lm - lq) < wd ? nd : den;
}

// --------------------------------------------------------------------------
// Histogram window close: FeatureParameterExtraction(self, 1), ns_core.c:337-517.
// Runs once per 500 frames per stream.  Zero bins cannot change any of the
// running sums / peaks, so only non-empty bins are visited, in bin order, which
// keeps the reference's sequential float sums and tie-breaking exactly.
struct PriorModel {
  float p0, p1, p3, p4, p5, p6;
};

// FLOW (ns_kernels1.hip's hand-off build): the histogram is read and cleared with agent-scope (sc1)
// accesses, like every other state access of that build.
template <bool FLOW>
__device__ __forceinline__ int hist_ld(const int32_t* p) {
  typedef __attribute__((address_space(1))) int gi32;
  if constexpr (FLOW) return __hip_atomic_load((const gi32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else return *p;
}
template <bool FLOW>
__device__ __forceinline__ void hist_st(int32_t* p, int v) {
  typedef __attribute__((address_space(1))) int gi32;
  if constexpr (FLOW) __hip_atomic_store((gi32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else *p = v;
}

template <bool FLOW = false>
__device__ inline __attribute__((noinline)) PriorModel close_histogram_window(int32_t* __restrict__ hist, int lane,
                                                          int updateWindow, bool zero_after,
                                                          PriorModel pm) {
  // ---- LRT histogram, :340-373
  float avgHistLrt = 0.f, avgHistLrtCompl = 0.f, avgSquareHistLrt = 0.f;
  int numHistLrt = 0;
  for (int r = 0; r < 16; ++r) {
    const int i = r * 64 + lane;
    const int v = i < kHist ? hist_ld<FLOW>(hist + i) : 0;
    unsigned long long m = __ballot(v != 0);
    while (m) {
      const int p = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int hv = __shfl(v, p, 64);
      const float binMid = ((float)(r * 64 + p) + 0.5f) * 0.1f;
      if (binMid <= 1.f) {
        avgHistLrt += hv * binMid;
        numHistLrt += hv;
      }
      avgSquareHistLrt += hv * binMid * binMid;
      avgHistLrtCompl += hv * binMid;
    }
  }
  if (numHistLrt > 0) avgHistLrt = avgHistLrt / ((float)numHistLrt);
  avgHistLrtCompl = avgHistLrtCompl / ((float)updateWindow);
  avgSquareHistLrt = avgSquareHistLrt / ((float)updateWindow);
  const float fluctLrt = avgSquareHistLrt - avgHistLrt * avgHistLrtCompl;
  if (fluctLrt < 0.05f) {
    pm.p0 = 1.f;
  } else {
    pm.p0 = 1.2f * avgHistLrt;
    if (pm.p0 < 0.2f) pm.p0 = 0.2f;
    if (pm.p0 > 1.f) pm.p0 = 1.f;
  }
  // ---- two dominant peaks of the flatness and difference histograms, :378-432
  float pos1[2], pos2[2];
  int wt1[2], wt2[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int32_t* hh = hist + (k + 1) * kHistStride;
    const float binSize = k == 0 ? 0.05f : 0.1f;
    int maxPeak1 = 0, maxPeak2 = 0;
    pos1[k] = 0.f;
    pos2[k] = 0.f;
    wt1[k] = 0;
    wt2[k] = 0;
    for (int r = 0; r < 16; ++r) {
      const int i = r * 64 + lane;
      const int v = i < kHist ? hist_ld<FLOW>(hh + i) : 0;
      unsigned long long m = __ballot(v != 0);
      while (m) {
        const int p = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int hv = __shfl(v, p, 64);
        const float binMid = ((float)(r * 64 + p) + 0.5f) * binSize;
        if (hv > maxPeak1) {
          maxPeak2 = maxPeak1;
          wt2[k] = wt1[k];
          pos2[k] = pos1[k];
          maxPeak1 = hv;
          wt1[k] = hv;
          pos1[k] = binMid;
        } else if (hv > maxPeak2) {
          maxPeak2 = hv;
          wt2[k] = hv;
          pos2[k] = binMid;
        }
      }
    }
  }
  const int thresWeight = (int)(0.3 * updateWindow);  // :67-70
  // ---- flatness, :435-463
  int useFlat = 1;
  if ((fabsf(pos2[0] - pos1[0]) < 2 * 0.05f) && (wt2[0] > 0.5f * wt1[0])) {
    wt1[0] += wt2[0];
    pos1[0] = 0.5f * (pos1[0] + pos2[0]);
  }
  if (wt1[0] < thresWeight || pos1[0] < 0.6f) useFlat = 0;
  if (useFlat == 1) {
    pm.p1 = 0.9f * pos1[0];
    if (pm.p1 < 0.1f) pm.p1 = 0.1f;
    if (pm.p1 > 0.95f) pm.p1 = 0.95f;
  }
  // ---- template difference, :467-498
  int useDiff = 1;
  if ((fabsf(pos2[1] - pos1[1]) < 2 * 0.1f) && (wt2[1] > 0.5f * wt1[1])) {
    wt1[1] += wt2[1];
    pos1[1] = 0.5f * (pos1[1] + pos2[1]);
  }
  pm.p3 = 1.2f * pos1[1];
  if (wt1[1] < thresWeight) useDiff = 0;
  if (pm.p3 < 0.16f) pm.p3 = 0.16f;
  if (pm.p3 > 1.f) pm.p3 = 1.f;
  if (fluctLrt < 0.05f) useDiff = 0;
  const float featureSum = (float)(1 + useFlat + useDiff);  // :504-507
  pm.p4 = 1.f / featureSum;
  pm.p5 = ((float)useFlat) / featureSum;
  pm.p6 = ((float)useDiff) / featureSum;
  if (zero_after) {  // :510-516
    for (int k = 0; k < 3; ++k)
      for (int r = 0; r < 16; ++r) hist_st<FLOW>(hist + k * kHistStride + r * 64 + lane, 0);
  }
  return pm;
}

// ---- the wave-uniform scalar sections of a frame step ----------------------------------------------------------------
// One value per stream, whatever the lane layout: each section of the reference is ONE function here for the frame
// kernels to call.  Inputs and results go by value; inside is arithmetic only -- no lane index, no LDS, no state access.
// A kernel reads and commits its scalar row itself, chooses the lanes that evaluate, and keeps the cross-lane steps (the
// sums in front, the tanh on lanes 0..2, the broadcasts).  NB: the geometry's bin count, so that the divisions by a
// constant stay what they are.  A call must leave a kernel's listing what it was (tools/listing_diff.py): where it does
// not, that kernel keeps the section's text (ns_kernels.hip: four of them).

// Pink-noise fit of the start-up model, its scalar part (ns_core.c:1098-1100, 1109-1149): from the two sums over the
// bins (log magn, log i * log magn) to the white level and the fit's two accumulators.  (The parametric model built from
// them, :1150-1156, the tanh arguments of the prior-model map, :696-725, and the histogram increment's per-slot
// constants, :309-334, stay in the kernels: as functions they change the listings of ns_kernels1.hip and ns_kernels2.hip.)
struct NsPinkFit {
  float whiteNoiseLevel, pinkNoiseNumerator, pinkNoiseExp;
};
template <int NB>
__device__ __forceinline__ NsPinkFit ns_pink_fit(const NsTables* T, float whiteNoiseLevel, float pinkNoiseNumerator,
                                                 float pinkNoiseExp, float sumMagn, float overdrive,
                                                 float sum_log_magn, float sum_log_i_log_magn, int blockInd) {
  static_assert(NB == kBins || NB == 65, "the two geometries whose sums over log i the tables hold");
  const float sum_log_i = NB == kBins ? T->sum_log_i : T->sum_log_i8;
  const float sum_log_i_square = NB == kBins ? T->sum_log_i_square : T->sum_log_i_square8;
  whiteNoiseLevel += ns_div_bins<NB>(sumMagn) * overdrive;
  float tmpFloat1 = sum_log_i_square * ((float)(NB - NS_START_BAND));
  tmpFloat1 -= (sum_log_i * sum_log_i);
  float tmpFloat2 = (sum_log_i_square * sum_log_magn - sum_log_i * sum_log_i_log_magn);
  float tmpFloat3 = tmpFloat2 / tmpFloat1;
  if (tmpFloat3 < 0.f) tmpFloat3 = 0.f;
  pinkNoiseNumerator += tmpFloat3;
  tmpFloat2 = (sum_log_i * sum_log_magn);
  tmpFloat2 -= ((float)(NB - NS_START_BAND)) * sum_log_i_log_magn;
  tmpFloat3 = tmpFloat2 / tmpFloat1;
  if (tmpFloat3 < 0.f) tmpFloat3 = 0.f;
  if (tmpFloat3 > 1.f) tmpFloat3 = 1.f;
  pinkNoiseExp += tmpFloat3;
  return {whiteNoiseLevel, pinkNoiseNumerator, pinkNoiseExp};
}
// Start-up average of the signal energy, featureData[5] (ns_core.c:1165-1169).
__device__ __forceinline__ float ns_startup_fd5(float fd5, float signalEnergy, int blockInd) {
  if (blockInd < NS_END_STARTUP_LONG) {
    fd5 *= blockInd;
    fd5 += signalEnergy;
    fd5 /= (blockInd + 1);
  }
  return fd5;
}

// Spectral flatness once its sums are in (ns_core.c:541-555): the exponential's argument and the denominator, then --
// the kernel evaluates the exponential where it likes -- the time-averaged feature, featureData[0].
struct NsFlatArgs {
  float arg, den;
};
template <int NB>
__device__ __forceinline__ NsFlatArgs ns_flatness_args(float sumLogMagn1, float sumMagn, float magn0) {
  float num = sumLogMagn1;  // over bins 1 .. NB - 1
  float den = sumMagn - magn0;
  den = ns_div_bins<NB>(den);
  num = ns_div_bins<NB>(num);
  return {num, den};
}
// (the _q forms take a quotient the caller has formed: ns_kernels1.hip divides two independent wave-uniform quotients
// at a time, ns_device.h fdiv2)
__device__ __forceinline__ float ns_flatness_update_q(float fd0, float spectralTmp) {
  fd0 += NS_SPECT_FL_TAVG * (spectralTmp - fd0);
  return fd0;
}
__device__ __forceinline__ float ns_flatness_update(float fd0, float expArg, float den) {
  return ns_flatness_update_q(fd0, fdiv(expArg, den));
}

// Spectral difference once its covariance and variances (sums over the bins, divided by their count) are in
// (ns_core.c:628-634): the time-averaged feature, featureData[4].  fd5: after ns_startup_fd5.
// Its two quotients are n1 / d1 and (varMagn - n1 / d1) / d2:
struct NsDiffArgs {
  float n1, d1, d2;
};
__device__ __forceinline__ NsDiffArgs ns_spectral_diff_args(float covMagnPause, float varPause, float fd5) {
  return {covMagnPause * covMagnPause, varPause + 0.0001f, fd5 + 0.0001f};
}
__device__ __forceinline__ float ns_spectral_diff_q(float fd4, float avgDiffNormMagn) {
  fd4 += NS_SPECT_DIFF_TAVG * (avgDiffNormMagn - fd4);
  return fd4;
}
__device__ __forceinline__ float ns_spectral_diff(float covMagnPause, float varPause, float varMagn, float fd4,
                                                  float fd5) {
  float avgDiffNormMagn = varMagn - fdiv(covMagnPause * covMagnPause, varPause + 0.0001f);
  avgDiffNormMagn = fdiv(avgDiffNormMagn, fd5 + 0.0001f);
  return ns_spectral_diff_q(fd4, avgDiffNormMagn);
}

// Feature-window bookkeeping behind a close (ns_core.c:773-788): the window reopens with modelUpdatePars[1] frames,
// a one-shot update (flag 1) switches itself off, a running one averages the window's energy into featureData[5].
struct NsWindowOpen {
  int mup0, mup3;
  float fd5, fd6;
};
__device__ __forceinline__ NsWindowOpen ns_window_reopen(int updateParsFlag, int mup1, float fd5, float fd6) {
  int mup0 = updateParsFlag;
  if (updateParsFlag == 1) {
    mup0 = 0;
  } else {
    fd6 = fd6 / ((float)mup1);
    fd5 = 0.5f * (fd6 + fd5);
    fd6 = 0.f;
  }
  return {mup0, mup1, fd5, fd6};
}

// The prior-model map behind its three tanh (ns_core.c:698-749): each tanh's indicator, indPrior, the update of
// priorSpeechProb and its clamps.
__device__ __forceinline__ float ns_prior_indicator(float th) { return 0.5f * (th + 1.f); }
__device__ __forceinline__ float ns_prior_update(float priorSpeechProb, PriorModel pm, float indicator0,
                                                 float indicator1, float indicator2) {
  const float indPrior = pm.p4 * indicator0 + pm.p5 * indicator1 + pm.p6 * indicator2;
  priorSpeechProb += NS_PRIOR_UPDATE * (indPrior - priorSpeechProb);
  if (priorSpeechProb > 1.f) priorSpeechProb = 1.f;
  if (priorSpeechProb < 0.01f) priorSpeechProb = 0.01f;
  return priorSpeechProb;
}

// Energy-based gain compensation (ns_core.c:1321-1342): the output's scale factor from the frame's energy in front of
// the filter (energy1) and behind it (energy2).  WAVE_SQRT: the square root in its wave-level form (fsqrt_wave) and
// 1 / gain through the reciprocal chain (frcp) -- the forms of ns_kernels1.hip; the other kernels' listings stay.
template <bool WAVE_SQRT = false>
__device__ __forceinline__ float ns_gain_factor(float energy2, float energy1, float denoiseBound,
                                                float priorSpeechProb) {
  float factor1 = 1.f, factor2 = 1.f;
  const float ratio = fdiv(energy2, energy1 + 1.f);
  float gain = WAVE_SQRT ? fsqrt_wave(ratio) : fsqrt(ratio);
  if (gain > NS_B_LIM) {
    factor1 = 1.f + 1.3f * (gain - NS_B_LIM);
    if (gain * factor1 > 1.f) factor1 = WAVE_SQRT ? frcp(gain) : fdiv(1.f, gain);  // (equal on every float)
  }
  if (gain < NS_B_LIM) {
    if (gain <= denoiseBound) gain = denoiseBound;
    factor2 = 1.f - 0.3f * (NS_B_LIM - gain);
  }
  return priorSpeechProb * factor1 + (1.f - priorSpeechProb) * factor2;
}

}  // namespace aspns_dev
