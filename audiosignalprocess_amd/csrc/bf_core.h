// bf_core.h -- webrtc::Beamformer (modules/audio_processing/beamformer/) over common_audio's LappedTransform,
// Blocker and WindowGenerator, restated once for the kernel (bf_kernels.hip), the host API (bf_api.hip) and the
// CPU build (bf_restate.cpp).
//
// A group Grp{lane, n} of ts_core.h runs one stream: n = 64 lanes of ONE wave on the device, n = 1 on the CPU.
// The transforms are ts_core.h's rdft (the Ooura transform, bit for bit), repacked as the specification does:
// bin 0 = (a[0], 0), bin k = (a[2k], -a[2k+1]), bin 128 = (a[1], 0); the inverse packs back, transforms and
// scales by 2.0f / 256.  The mask stage runs one bin per lane; every sum inside a bin (the quadratic forms, the
// dot products, the channel sum of ApplyMasks) and the two band means keep the reference's sequential order in
// one lane.  Complex products are (ac - bd, ad + bc) in float, unfused (-ffp-contract=off); conjugation and the
// packing's negations are exact, so a - (-b) is written a + b.  std::abs(complex<float>) is glibc's hypotf,
// evaluated here in fp64 with one rounding (tests/test_bf_host.py compares it with the host's libm).
//
// Initialize (make_tables) is host only and runs once per batch: it follows the reference's expressions with its
// float / double types on std::complex<float> and calls the host libm (j0, sin, cos, pow, sqrt) as it does.
#ifndef ASP_BF_CORE_H_
#define ASP_BF_CORE_H_

#include <math.h>
#include <stdint.h>

#include "bf_layout.h"
#include "ts_core.h"

#define BF_HD TS_HD
#if defined(__clang__)
#define BF_UNROLL _Pragma("unroll")
#else
#define BF_UNROLL
#endif

namespace aspbf {

using aspts::Grp;
using aspts::grp_sync;

// ------------------------------------------------------------------------------------------- per-chunk path
// glibc's hypotf for finite arguments: the exact squares summed in fp64, its square root, one rounding to float
BF_HD float bf_hypotf(float x, float y) {
  const uint32_t ax = aspts::as_u32(x) & 0x7fffffffu, ay = aspts::as_u32(y) & 0x7fffffffu;
  if (ax >= 0x7f800000u || ay >= 0x7f800000u) {
    if (ax == 0x7f800000u || ay == 0x7f800000u) return aspts::as_f32(0x7f800000u);
    return x + y;
  }
  return (float)sqrt((double)x * (double)x + (double)y * (double)y);
}

BF_HD float bf_max(float a, float b) { return a < b ? b : a; }  // std::max

// bin i of a transformed block in rdft's packing, as the specification's CCS value
BF_HD void spec_bin(const float* a, int i, float& re, float& im) {
  if (i == 0) {
    re = a[0];
    im = 0.f;
  } else if (i == kBins - 1) {
    re = a[1];
    im = 0.f;
  } else {
    re = a[2 * i];
    im = -a[2 * i + 1];
  }
}

// Norm(mat, eig) (beamformer.cc:79-101): the real part of conj(e) * mat * transpose(e); i outer, j inner,
// first_product reset per i.  conj_mat: the matrix is the stored one conjugated (the reflected interferer).
template <int M>
BF_HD float quad_form(const float* cov, int bin, bool conj_mat, const float* er, const float* ei) {
  float sr = 0.f;
BF_UNROLL
  for (int i = 0; i < M; ++i) {
    float fr = 0.f, fi = 0.f;
BF_UNROLL
    for (int j = 0; j < M; ++j) {
      const float* m = cov + ((size_t)(j * M + i) * kBins + bin) * 2;
      const float mr = m[0], mi = conj_mat ? -m[1] : m[1];
      fr += er[j] * mr + ei[j] * mi;  // conj(e[j]) * m
      fi += er[j] * mi - ei[j] * mr;
    }
    sr += fr * er[i] - fi * ei[i];
  }
  return sr;
}

// CalculatePostfilterMask (beamformer.cc:397-415)
BF_HD float postfilter_mask(float rpsim, float rpsiw, float ratio_rxiw_rxim, float rmw_r, float mask_threshold) {
  const float ratio = rpsiw / rpsim;
  const float numerator = rmw_r - ratio;
  const float denominator = ratio_rxiw_rxim - ratio;
  float mask = 1.f;
  if (denominator > mask_threshold) {
    const float lambda = numerator / denominator;
    mask = bf_max(lambda * ratio_rxiw_rxim / rmw_r, kMaskMinimum);
  }
  return mask;
}

// the mask of bin i from the M transformed blocks (ProcessAudioBlock's loop body, beamformer.cc:346-375)
template <int M>
BF_HD float bin_mask(const BfTables& tb, const float* spec, int i) {
  float er[M], ei[M];
  float dot = 0.f;
BF_UNROLL
  for (int c = 0; c < M; ++c) {
    spec_bin(spec + c * kFft, i, er[c], ei[c]);
    dot += er[c] * er[c] + ei[c] * ei[c];  // ConjugateDotProduct(eig_m_, eig_m_): the imaginary part is x - x
  }
  const float norm = sqrtf(dot);
  if (norm != 0.f) {
    const float inv = 1.f / norm;
BF_UNROLL
    for (int c = 0; c < M; ++c) {
      er[c] *= inv;
      ei[c] *= inv;
    }
  }
  const float rxim = quad_form<M>(tb.tcov, i, false, er, ei);
  float ratio_rxiw_rxim = 0.f;
  if (rxim != 0.f) ratio_rxiw_rxim = tb.rxiw[i] / rxim;
  float pr = 0.f, pi = 0.f;  // ConjugateDotProduct(delay_sum_masks_[i], eig_m_)
BF_UNROLL
  for (int c = 0; c < M; ++c) {
    const float* d = tb.dsm + ((size_t)c * kBins + i) * 2;
    pr += d[0] * er[c] + d[1] * ei[c];
    pi += d[0] * ei[c] - d[1] * er[c];
  }
  const float rmw = bf_hypotf(pr, pi);
  const float rmw_r = rmw * rmw;  // (r, 0) * (r, 0)
  const float thr = tb.thr[i];
  const float m0 = postfilter_mask(quad_form<M>(tb.icov, i, false, er, ei), tb.rpsiw[i], ratio_rxiw_rxim, rmw_r, thr);
  const float m1 = postfilter_mask(quad_form<M>(tb.icov, i, true, er, ei), tb.rrpsiw[i], ratio_rxiw_rxim, rmw_r, thr);
  return m0 * m1;
}

// One block of the lapped transform at `first` of the input buffer: window, M forward transforms,
// ProcessAudioBlock, the inverse transform, window, overlap-add (blocker.cc:192-223, lapped_transform.cc:21-51,
// beamformer.cc:332-395).  in [M][384], out [384].
template <int M>
BF_HD void process_block(const BfParams& p, const BfTables& tb, AspBfState& st, BfWork<M>& w, const float* in,
                         float* out, int first, bool high, const Grp& g) {
  float* spec = &w.spec[0][0];
  TS_PAR(t, M * kFft) {
    const int c = t / kFft, j = t - c * kFft;
    spec[t] = in[c * kBuf + first + j] * tb.window[j];
  }
  grp_sync(g);
  for (int c = 0; c < M; ++c) aspts::rdft(kFft, 1, spec + c * kFft, tb.w, g);

  float* mask = st.postfilter_masks[st.current_block_ix];
  TS_PAR(i, kBins) mask[i] = bin_mask<M>(tb, spec, i);
  grp_sync(g);

  // EstimateTargetPresence: the order statistic at index 65 by counting ranks (any exact selection gives the
  // value std::nth_element leaves there; the masks are finite)
  TS_PAR(i, kBins) {
    const float v = mask[i];
    int rank = 0;
    for (int j = 0; j < kBins; ++j) {
      const float u = mask[j];
      rank += (u < v || (u == v && j < i)) ? 1 : 0;
    }
    if (rank == kMedianIx) w.sc.median = v;
  }
  grp_sync(g);
  if (g.lane == 0) {
    if (w.sc.median > kMaskTargetThreshold) {
      st.is_target_present = 1;
      st.interference_blocks_count = 0;
    } else {
      st.is_target_present = st.interference_blocks_count++ < p.hold ? 1 : 0;
    }
  }
  if (st.previous_block_ix >= 0) {  // ApplyDecay
    const float* prev = st.postfilter_masks[st.previous_block_ix];
    TS_PAR(i, kBins) mask[i] = bf_max(mask[i], prev[i] * p.decay);
  }
  grp_sync(g);
  // the two band means, each in one lane in ascending order; the low-frequency correction writes bins below the
  // mid band only, which the high band's mean (bins 64..112) does not read
  if (g.lane == 0) {  // ApplyLowFrequencyCorrection
    float m = 0.f;
    for (int i = p.mid_lo; i <= p.mid_hi; ++i) m += mask[i];
    m /= (float)(p.mid_hi - p.mid_lo + 1);
    for (int i = 0; i < p.mid_lo; ++i) mask[i] = m;
  }
  if (high && g.lane == (g.n > 1 ? 1 : 0)) {  // CalculateHighFrequencyMask
    float m = 0.f;
    for (int i = p.high_lo; i <= p.high_hi; ++i) m += mask[i];
    m /= (float)(p.high_hi - p.high_lo + 1);
    st.high_pass_postfilter_mask += m;
  }
  grp_sync(g);

  TS_PAR(f, kBins) {  // ApplyMasks, packed for the inverse transform
    float sr = 0.f, si = 0.f;
BF_UNROLL
    for (int c = 0; c < M; ++c) {
      float xr, xi;
      spec_bin(spec + c * kFft, f, xr, xi);
      const float* d = tb.dsm + ((size_t)c * kBins + f) * 2;
      sr += xr * d[0] - xi * d[1];
      si += xr * d[1] + xi * d[0];
    }
    sr *= mask[f];
    si *= mask[f];
    if (f == 0) {
      w.ob[0] = sr;
    } else if (f == kBins - 1) {
      w.ob[1] = sr;
    } else {
      w.ob[2 * f] = sr;
      w.ob[2 * f + 1] = -si;
    }
  }
  grp_sync(g);
  aspts::rdft(kFft, -1, w.ob, tb.w, g);
  TS_PAR(j, kFft) {
    const float y = w.ob[j] * (2.0f / kFft) * tb.window[j];
    out[first + j] = out[first + j] + y;
  }
  grp_sync(g);
  if (g.lane == 0) {
    st.previous_block_ix = st.current_block_ix;
    st.current_block_ix = (st.current_block_ix + 1) % 2;
    w.sc.nblocks++;
  }
  grp_sync(g);
}

// Beamformer::ProcessChunk over Blocker::ProcessChunk (beamformer.cc:289-330, blocker.cc:171-258).
// input [M][160]; high_input [M][160] or NULL; output [160]; high_output [160].
template <int M>
BF_HD void process_chunk(const BfParams& p, const BfTables& tb, AspBfState& st, BfWork<M>& w, float* in, float* out,
                         const float* input, const float* high_input, float* output, float* high_output,
                         const Grp& g) {
  const bool high = high_input != nullptr;
  TS_PAR(t, M * kChunk) {
    const int c = t / kChunk, j = t - c * kChunk;
    in[c * kBuf + kDelay + j] = input[t];
  }
  if (g.lane == 0) {
    w.sc.nblocks = 0;
    w.sc.old_high = st.high_pass_postfilter_mask;
    st.high_pass_postfilter_mask = 0.f;
  }
  grp_sync(g);
  int first = st.frame_offset;
  while (first < kChunk) {
    process_block<M>(p, tb, st, w, in, out, first, high, g);
    first += kShift;
  }
  TS_PAR(j, kChunk) output[j] = out[j];
  grp_sync(g);
  // the two buffer moves overlap: staged through the block memory, which is free between chunks
  float* stage = &w.spec[0][0];
  TS_PAR(t, M * kDelay) {
    const int c = t / kDelay, j = t - c * kDelay;
    stage[t] = in[c * kBuf + kChunk + j];
  }
  TS_PAR(j, kDelay) w.ob[j] = out[kChunk + j];
  grp_sync(g);
  TS_PAR(t, M * kDelay) {
    const int c = t / kDelay, j = t - c * kDelay;
    in[c * kBuf + j] = stage[t];
  }
  TS_PAR(j, kDelay) out[j] = w.ob[j];
  TS_PAR(j, kChunk) out[kDelay + j] = 0.f;
  if (g.lane == 0) st.frame_offset = first - kChunk;
  if (high) {
    if (g.lane == 0) {
      st.high_pass_postfilter_mask /= (float)w.sc.nblocks;
      float old = w.sc.old_high;
      if (st.previous_block_ix == -1) old = st.high_pass_postfilter_mask;
      const float ramp_inc = (st.high_pass_postfilter_mask - old) / (float)kChunk;
      for (int i = 0; i < kChunk; ++i) {
        old += ramp_inc;
        w.ramp[i] = old;
      }
    }
    grp_sync(g);
    TS_PAR(i, kChunk) {
      float sum = 0.f;
BF_UNROLL
      for (int c = 0; c < M; ++c) sum += high_input[c * kChunk + i];
      high_output[i] = sum / (float)M * w.ramp[i];
    }
  }
  grp_sync(g);
}

// the state after the constructor and Initialize; the caller zeroes the stream's buffer array
BF_HD void init_state(AspBfState& s, int M, int hold) {
  s.num_mics = M;
  s.frame_offset = 0;
  s.current_block_ix = 0;
  s.previous_block_ix = -1;
  s.is_target_present = 0;
  s.interference_blocks_count = hold;
  s.high_pass_postfilter_mask = 0.f;
  s.reserved = 0;
  for (int r = 0; r < 2; ++r)
    for (int i = 0; i < kBins; ++i) s.postfilter_masks[r][i] = 0.f;
}

}  // namespace aspbf

// ------------------------------------------------------------------------------------------- Initialize (host)
#include <complex>
#include <vector>

namespace aspbf {

typedef std::complex<float> cf;

struct HostTables {
  int M = 0;
  float mic_spacing = 0.f;
  std::vector<float> t[kTabCount];  // the reference's element order (include/asp_bf.h)
};

// WindowGenerator::KaiserBesselDerived (window_generator.cc:25-69)
inline cf kbd_i0(cf x) {
  cf y = x / 3.75f;
  y *= y;
  return 1.0f + y * (3.5156229f + y * (3.0899424f + y * (1.2067492f + y * (0.2659732f + y * (0.360768e-1f + y * 0.45813e-2f)))));
}
inline void make_kbd_window(float alpha, int length, float* window) {
  const int half = (length + 1) / 2;
  float sum = 0.0f;
  for (int i = 0; i <= half; ++i) {
    cf r = (4.0f * i) / length - 1.0f;
    sum += kbd_i0(static_cast<float>(M_PI) * alpha * std::sqrt(1.0f - r * r)).real();
    window[i] = sum;
  }
  for (int i = length - 1; i >= half; --i) {
    window[length - i - 1] = sqrtf(window[length - i - 1] / sum);
    window[i] = window[length - i - 1];
  }
  if (length % 2 == 1) window[half - 1] = sqrtf(window[half - 1] / sum);
}

// Beamformer::MicSpacingFromGeometry (beamformer.cc:477-488); false where the reference CHECKs
inline bool mic_spacing_from_geometry(const float* xyz, int M, float* spacing) {
  float mic_spacing = 0.f;
  for (int i = 0; i < 3; ++i) {
    const float difference = xyz[3 + i] - xyz[i];
    for (int j = 2; j < M; ++j)
      if (!(xyz[3 * j + i] - xyz[3 * (j - 1) + i] - difference < 1e-6)) return false;
    mic_spacing += difference * difference;
  }
  *spacing = sqrt((double)mic_spacing);
  return true;
}

// CovarianceMatrixGenerator::PhaseAlignmentMasks (covariance_matrix_generator.cc:130-152): row vector [M]
inline void phase_alignment_masks(int frequency_bin, int fft_size, int sample_rate, float sound_speed, float mic_spacing,
                                  int M, float sin_angle, cf* mat) {
  const float freq_in_hertz = (static_cast<float>(frequency_bin) / fft_size) * sample_rate;
  for (int c_ix = 0; c_ix < M; ++c_ix) {
    const float distance = mic_spacing * c_ix * sin_angle * -1.f;
    const float phase_shift = 2 * M_PI * distance * freq_in_hertz / sound_speed;
    mat[c_ix] = cf(cos((double)phase_shift), sin((double)phase_shift));
  }
}

// CovarianceMatrixGenerator::Boxcar (:33-54): [M][M]
inline void boxcar(float wave_number, int M, float mic_spacing, float half_width, cf* mat) {
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) {
      if (i == j) {
        mat[i * M + j] = cf(2.f * half_width, 0.f);
      } else {
        const float factor = (j - i) * wave_number * mic_spacing;
        const float boxcar_real = 2.f * sin((double)(factor * half_width)) / factor;
        mat[i * M + j] = cf(boxcar_real, 0.f);
      }
    }
}

// CovarianceMatrixGenerator::DCCovarianceMatrix (:110-128)
inline void dc_covariance(int M, float half_width, cf* mat) {
  const float diagonal_value = 1 - (2 * half_width);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) mat[i * M + j] = i == j ? cf(diagonal_value, 0.f) : cf(0.f, 0.f);
}

inline cf trace(const cf* mat, int M) {
  cf t = 0;
  for (int i = 0; i < M; ++i) t += mat[i * M + i];
  return t;
}
// 1.f / z as the reference's build divides complex<float> (libgcc's __divsc3: Smith's algorithm, the larger
// component of z divides first), for the finite non-zero divisors of these tables (a norm, a trace: the imaginary
// part is exactly 0, so this is 1.f / z.real()).  Written out because the quotient is the complex runtime's
// otherwise: compiler-rt's __divsc3, which hipcc links into the library, forms c * c + d * d in float and gives
// other tables at 2, 3, 6 and 8 microphones.
inline cf recip(cf z) {
  const float a = 1.f, b = 0.f, c = z.real(), d = z.imag();
  if (fabsf(c) < fabsf(d)) {
    const float ratio = c / d, denom = c * ratio + d;
    return cf((a * ratio + b) / denom, (b * ratio - a) / denom);
  }
  const float ratio = d / c, denom = d * ratio + c;
  return cf((b * ratio + a) / denom, (b - a * ratio) / denom);
}
template <typename S>
inline void scale(cf* mat, int count, const S& scalar) {
  for (int i = 0; i < count; ++i) mat[i] *= scalar;
}

// Norm (beamformer.cc:79-101) on a row vector [M] and a matrix [M][M]
inline float host_norm(const cf* mat, const cf* norm_mat, int M) {
  cf first_product = cf(0.f, 0.f), second_product = cf(0.f, 0.f);
  for (int i = 0; i < M; ++i) {
    for (int j = 0; j < M; ++j) {
      cf cur_norm_element = std::conj(norm_mat[j]);
      cf cur_mat_element = mat[j * M + i];
      first_product += cur_norm_element * cur_mat_element;
    }
    second_product += first_product * norm_mat[i];
    first_product = 0.f;
  }
  return second_product.real();
}

inline void store(std::vector<float>& dst, const std::vector<cf>& src) {
  dst.resize(2 * src.size());
  for (size_t i = 0; i < src.size(); ++i) {
    dst[2 * i] = src[i].real();
    dst[2 * i + 1] = src[i].imag();
  }
}

// The constructor's and Initialize's checks and tables (beamformer.cc:128-287).  Returns NULL, or the reason the
// call is refused.
inline const char* make_tables(HostTables& h, BfParams& p, int num_mics, const float* xyz, int chunk_size_ms,
                               int sample_rate_hz) {
  const float kAlpha = 1.5f, kSpeedOfSound = 340, kTargetAngle = 0.f, kInterfAngle = static_cast<float>(M_PI) / 4.f;
  const float kBalance = 0.2f, kBeamwidthConstant = 0.00001f, kBoxcarHalfWidth = 0.001f, kCovUniformGapHalfWidth = 0.001f;
  const float kHalfLifeSeconds = 0.05f, kHoldTargetSeconds = 0.25f;
  if (num_mics < kMinM || num_mics > kMaxM) return "the microphone count must be 2 to 8";
  if (!xyz) return "NULL geometry";
  if (sample_rate_hz != 16000)
    return "the band rate must be 16000 Hz (at 8 kHz the reference's own bound on high_frequency_upper_bin_bound_ "
           "does not hold; 32 and 48 kHz streams pass their bands)";
  if (chunk_size_ms != 10) return "the chunk must be 10 ms";
  const int M = num_mics;
  float mic_spacing;
  if (!mic_spacing_from_geometry(xyz, M, &mic_spacing)) return "the geometry is not a uniform linear array";
  h.M = p.M = M;
  h.mic_spacing = mic_spacing;
  const int sample_rate_hz_ = sample_rate_hz;
  p.decay = pow(2.0, (double)((kFft / -2.f) / (sample_rate_hz_ * kHalfLifeSeconds)));
  p.mid_lo = (int)floorf((float)(250 * kFft / sample_rate_hz_) + 0.5f);
  p.mid_hi = (int)floorf((float)(400 * kFft / sample_rate_hz_) + 0.5f);
  p.high_lo = (int)floorf((float)(4000 * kFft / sample_rate_hz_) + 0.5f);
  p.high_hi = (int)floorf((float)(7000 * kFft / sample_rate_hz_) + 0.5f);
  p.hold = kHoldTargetSeconds * 2 * sample_rate_hz / kFft;
  if (!(p.mid_hi <= kBins && p.mid_lo < p.mid_hi && p.high_hi <= kBins && p.high_lo < p.high_hi))
    return "the bin bounds do not fit the transform";
  h.t[kTabDecay].assign(1, p.decay);
  h.t[kTabWindow].resize(kFft);
  make_kbd_window(kAlpha, kFft, h.t[kTabWindow].data());

  std::vector<float>& wave_numbers = h.t[kTabWave];
  wave_numbers.resize(kBins);
  h.t[kTabThr].resize(kBins);
  for (int i = 0; i < kBins; ++i) {
    const float freq_hz = (static_cast<float>(i) / kFft) * sample_rate_hz_;
    wave_numbers[i] = 2 * M_PI * freq_hz / kSpeedOfSound;
  }
  for (int i = 0; i < kBins; ++i) h.t[kTabThr][i] = M * M * kBeamwidthConstant * wave_numbers[i] * wave_numbers[i];

  const int MM = M * M;
  std::vector<cf> dsm((size_t)kBins * M), tcov((size_t)kBins * MM), icov((size_t)kBins * MM), rcov((size_t)kBins * MM);
  // InitDelaySumMasks
  const float sin_target = sin((double)kTargetAngle);
  for (int f = 0; f < kBins; ++f) {
    cf* d = &dsm[(size_t)f * M];
    phase_alignment_masks(f, kFft, sample_rate_hz_, kSpeedOfSound, mic_spacing, M, sin_target, d);
    cf dot = cf(0.f, 0.f);
    for (int i = 0; i < M; ++i) dot += std::conj(d[i]) * d[i];
    const cf norm_factor = std::sqrt(dot);
    scale(d, M, recip(norm_factor));
  }
  // InitTargetCovMats
  for (int i = 0; i < kBins; ++i) {
    cf* m = &tcov[(size_t)i * MM];
    if (i == 0)
      dc_covariance(M, kBoxcarHalfWidth, m);
    else
      boxcar(wave_numbers[i], M, mic_spacing, kBoxcarHalfWidth, m);
    const cf normalization_factor = trace(m, M);
    scale(m, MM, recip(normalization_factor));
  }
  // InitInterfCovMats
  {
    cf* m = &icov[0];
    dc_covariance(M, kCovUniformGapHalfWidth, m);
    const cf normalization_factor = trace(m, M);
    scale(m, MM, recip(normalization_factor));
  }
  std::vector<cf> uniform(MM), angled(MM), box(MM), vec(M), vec_t(M);
  for (int i = 1; i < kBins; ++i) {
    const float wave_number = wave_numbers[i];
    // GappedUniformCovarianceMatrix
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < M; ++c) {
        const float x = (c - r) * wave_number * mic_spacing;
        const float bessel = j0((double)x);
        uniform[r * M + c] = bessel;
      }
    boxcar(wave_number, M, mic_spacing, kCovUniformGapHalfWidth, box.data());
    for (int k = 0; k < MM; ++k) uniform[k] -= box[k];
    // AngledCovarianceMatrix
    phase_alignment_masks(i, kFft, sample_rate_hz_, kSpeedOfSound, mic_spacing, M, sin((double)kInterfAngle), vec.data());
    for (int k = 0; k < M; ++k) vec_t[k] = vec[k];
    for (int k = 0; k < M; ++k) vec[k] = std::conj(vec[k]);
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < M; ++c) {
        cf cur_element = 0;
        cur_element += vec_t[r] * vec[c];
        angled[r * M + c] = cur_element;
      }
    cf normalization_factor = trace(uniform.data(), M);
    scale(uniform.data(), MM, recip(normalization_factor));
    normalization_factor = trace(angled.data(), M);
    scale(angled.data(), MM, recip(normalization_factor));
    scale(uniform.data(), MM, 1 - kBalance);
    scale(angled.data(), MM, kBalance);
    cf* m = &icov[(size_t)i * MM];
    for (int k = 0; k < MM; ++k) {
      m[k] = uniform[k];
      m[k] += angled[k];
    }
  }
  for (size_t k = 0; k < icov.size(); ++k) rcov[k] = std::conj(icov[k]);

  h.t[kTabRxiw].resize(kBins);
  h.t[kTabRpsiw].resize(kBins);
  h.t[kTabRrpsiw].resize(kBins);
  for (int i = 0; i < kBins; ++i) {
    const cf* d = &dsm[(size_t)i * M];
    h.t[kTabRxiw][i] = host_norm(&tcov[(size_t)i * MM], d, M);
    h.t[kTabRpsiw][i] = host_norm(&icov[(size_t)i * MM], d, M);
    h.t[kTabRrpsiw][i] = host_norm(&rcov[(size_t)i * MM], d, M);
  }
  store(h.t[kTabDsm], dsm);
  store(h.t[kTabTcov], tcov);
  store(h.t[kTabIcov], icov);
  return nullptr;
}

// the kernel's table array (bf_layout.h) from the reference-order tables
inline void pack_tables(const HostTables& h, std::vector<float>& pack) {
  const int M = h.M;
  pack.assign((size_t)pack_floats(M), 0.f);
  float* p = pack.data();
  const BfTables v = view_tables(p, M);
  for (int j = 0; j < kFft; ++j) p[j] = h.t[kTabWindow][j];
  aspts::make_fft_w(kFft, p + kFft);
  for (int i = 0; i < kBins; ++i) {
    const_cast<float*>(v.thr)[i] = h.t[kTabThr][i];
    const_cast<float*>(v.rxiw)[i] = h.t[kTabRxiw][i];
    const_cast<float*>(v.rpsiw)[i] = h.t[kTabRpsiw][i];
    const_cast<float*>(v.rrpsiw)[i] = h.t[kTabRrpsiw][i];
    for (int c = 0; c < M; ++c)
      for (int k = 0; k < 2; ++k) const_cast<float*>(v.dsm)[((size_t)c * kBins + i) * 2 + k] = h.t[kTabDsm][((size_t)i * M + c) * 2 + k];
    for (int e = 0; e < M * M; ++e)
      for (int k = 0; k < 2; ++k) {
        const_cast<float*>(v.tcov)[((size_t)e * kBins + i) * 2 + k] = h.t[kTabTcov][((size_t)i * M * M + e) * 2 + k];
        const_cast<float*>(v.icov)[((size_t)e * kBins + i) * 2 + k] = h.t[kTabIcov][((size_t)i * M * M + e) * 2 + k];
      }
  }
}

}  // namespace aspbf
#endif  // ASP_BF_CORE_H_
