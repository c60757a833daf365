// ab_core.h -- the audio buffer's arithmetic, one source for the kernels (ab_kernels.hip) and the CPU build
// (ab_restate.cpp): the sample conversions of common_audio/include/audio_util.h, both StereoToMono forms of
// audio_buffer.cc, and the resampler's 32-tap convolution in the order of Convolve_SSE
// (common_audio/resampler/sinc_resampler_sse.cc:19-57).  Every function is one IEEE operation per reference
// operation, or integer arithmetic; compile without contraction (-ffp-contract=off).
#ifndef ASP_AB_CORE_H_
#define ASP_AB_CORE_H_

#include <stdint.h>

#if defined(__HIPCC__)
#define AB_HD __host__ __device__
#else
#define AB_HD
#endif

namespace aspab {

// FloatToFloatS16: v * (v > 0 ? 32767 : 32768); -0.0 stays -0.0
AB_HD inline float float_to_float_s16(float v) { return v * (v > 0 ? 32767.f : 32768.f); }

// FloatS16ToFloat: v * (v > 0 ? 1.f / 32767 : 1.f / 32768), the first constant rounded to float as the reference's
AB_HD inline float float_s16_to_float(float v) {
  const float kMaxInt16Inverse = 1.f / 32767.f, kMinInt16InverseNeg = 1.f / 32768.f;
  return v * (v > 0 ? kMaxInt16Inverse : kMinInt16InverseNeg);
}

// FloatS16ToS16: round half away from zero, clamp at 32766.5 / -32767.5 (IFChannelBuffer::RefreshI)
AB_HD inline int16_t float_s16_to_s16(float v) {
  const float kMaxRound = 32767 - 0.5f, kMinRound = -32768 + 0.5f;
  if (v > 0) return v >= kMaxRound ? (int16_t)32767 : (int16_t)(v + 0.5f);
  return v <= kMinRound ? (int16_t)-32768 : (int16_t)(v - 0.5f);
}

// IFChannelBuffer::RefreshF
AB_HD inline float s16_to_float_s16(int16_t v) { return (float)v; }

// StereoToMono<int16_t> and DeinterleaveFrom's downmix: the sum in int, the division truncating toward zero
AB_HD inline int16_t stereo_to_mono(int16_t l, int16_t r) { return (int16_t)(((int)l + (int)r) / 2); }
// StereoToMono<float>: one add, one division by (float)2
AB_HD inline float stereo_to_mono(float l, float r) { return (l + r) / 2.f; }

struct Quad {
  float a, b, c, d;
};

// One output sample of SincResampler::Resample: Convolve_SSE(x, k1, k2, factor) with f1 = (float)(1 - factor),
// f2 = (float)factor.  K(c) returns taps 4c .. 4c + 3 of a kernel row.  Four partial sums per kernel (tap i goes to
// sum i mod 4), the blend per partial sum, then (t2 + t0) + (t3 + t1).
template <class K1, class K2>
AB_HD inline float convolve32(const float* x, K1 k1, K2 k2, float f1, float f2) {
  float s1a = 0.f, s1b = 0.f, s1c = 0.f, s1d = 0.f, s2a = 0.f, s2b = 0.f, s2c = 0.f, s2d = 0.f;
#if defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < 8; ++c) {
    const Quad p = k1(c), q = k2(c);
    const float x0 = x[4 * c], x1 = x[4 * c + 1], x2 = x[4 * c + 2], x3 = x[4 * c + 3];
    s1a = s1a + x0 * p.a;
    s1b = s1b + x1 * p.b;
    s1c = s1c + x2 * p.c;
    s1d = s1d + x3 * p.d;
    s2a = s2a + x0 * q.a;
    s2b = s2b + x1 * q.b;
    s2c = s2c + x2 * q.c;
    s2d = s2d + x3 * q.d;
  }
  const float t0 = s1a * f1 + s2a * f2, t1 = s1b * f1 + s2b * f2;
  const float t2 = s1c * f1 + s2c * f2, t3 = s1d * f1 + s2d * f2;
  return (t2 + t0) + (t3 + t1);
}

}  // namespace aspab

#endif  // ASP_AB_CORE_H_
