// ts_core.h -- webrtc::TransientSuppressor (modules/audio_processing/transient/) restated once, for the
// kernel (ts_kernels.hip), the host API's tables (ts_api.hip) and the CPU build (ts_restate.cpp).
//
// A "group" G{lane, n} runs one stream: n = 64 lanes of a wave on the device, n = 1 on the CPU.  Loops over
// bins, samples and butterflies are strided by the group; the reference's serial float sums and the scalar
// state machine run on lane 0; grp_sync() separates the phases.  Every float operation is the reference's,
// in its order, unfused (-ffp-contract=off); the parallel phases only reorder independent operations.
//
// The specification is the reference built for x86-64: FIRFilter::Create picks
// FIRFilterSSE2 (four partial sums over j mod 4, then (l0 + l2) + (l1 + l3)), and cos / exp / pow on float
// arguments are libstdc++'s float overloads, i.e. glibc's cosf, expf, powf, and sincosf for the phase.  libm
// is not called here: ts_expf, ts_powf, ts_sinf and ts_cosf evaluate in fp64 with + and * and round once, on
// the CPU and on the GPU alike (the constants are those of the Arm optimized routines that glibc >= 2.28
// ships; tests/test_ts_host.py compares them with the host's libm).
#ifndef ASP_TS_CORE_H_
#define ASP_TS_CORE_H_

#include <float.h>
#include <stdint.h>

#include "ts_layout.h"

#if defined(__HIPCC__)
#define TS_HD __host__ __device__ inline
#else
#define TS_HD inline
#endif

namespace aspts {

struct Grp {
  int lane, n;
};
TS_HD void grp_sync(const Grp&) {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();
#endif
}
#define TS_PAR(i, count) for (int i = g.lane; i < (count); i += g.n)

TS_HD uint32_t as_u32(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
TS_HD float as_f32(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
TS_HD uint64_t as_u64(double d) { uint64_t u; __builtin_memcpy(&u, &d, 8); return u; }
TS_HD double as_f64(uint64_t u) { double d; __builtin_memcpy(&d, &u, 8); return d; }
TS_HD float ts_fabsf(float x) { return as_f32(as_u32(x) & 0x7fffffffu); }

// ------------------------------------------------------------------------------------------- transcendentals
constexpr float kPi = 3.14159265358979323846f;  // ts::kPi

// 2^(i / 32) as bits, less i << 47 (exp2f_data.c of the Arm optimized routines)
static constexpr uint64_t kExp2Tab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

// 2^(k / 32 + r) for kd = k + shift: the table entry times a cubic in r, |r| <= 1 / 64 (in units of 1 / 32
// for expf, whose polynomial is scaled accordingly)
TS_HD double exp2_tail(uint64_t ki, double r, double c0, double c1, double c2) {
  const uint64_t t = kExp2Tab[ki % 32] + (ki << 47);
  const double s = as_f64(t);
  const double z = c0 * r + c1;
  const double r2 = r * r;
  double y = c2 * r + 1.0;
  y = z * r2 + y;
  return y * s;
}

TS_HD float ts_expf(float x) {
  const uint32_t ix = as_u32(x), abstop = (ix >> 20) & 0x7ff;
  if (abstop >= 0x42b) {  // |x| >= 88 or NaN
    if (ix == 0xff800000u) return 0.0f;
    if (abstop >= 0x7f8) return x + x;
    if (x > 0x1.62e42ep6f) return as_f32(0x7f800000u);
    if (x < -0x1.9fe368p6f) return 0.0f;
    if (x < -0x1.9d1d9ep6f) return 0x1p-149f;  // the library's may-underflow return: 0x1.4p-75f squared
  }
  const double shift = 0x1.8p+52;
  const double z = 0x1.71547652b82fep+5 * (double)x;  // 32 / ln 2
  double kd = z + shift;
  const uint64_t ki = as_u64(kd);
  kd -= shift;
  const double r = z - kd;
  return (float)exp2_tail(ki, r, 0x1.c6af84b912394p-20, 0x1.ebfce50fac4f3p-13, 0x1.62e42ff0c52d6p-6);
}

// powf for x >= 0 (the callers' domain: x = 1 - detector_smoothed_, y = 50 or 200), finite y > 0
static constexpr double kLog2Tab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.efec65b963019p-2}, {0x1.571ed4aaf883dp+0, -0x1.b0b6832d4fca4p-2},
    {0x1.49539f0f010bp+0, -0x1.7418b0a1fb77bp-2},  {0x1.3c995b0b80385p+0, -0x1.39de91a6dcf7bp-2},
    {0x1.30d190c8864a5p+0, -0x1.01d9bf3f2b631p-2}, {0x1.25e227b0b8eap+0, -0x1.97c1d1b3b7afp-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.2f9e393af3c9fp-3}, {0x1.12358f08ae5bap+0, -0x1.960cbbf788d5cp-4},
    {0x1.0953f419900a7p+0, -0x1.a6f9db6475fcep-5}, {0x1p+0, 0x0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.338ca9f24f53dp-4},  {0x1.ca4b31f026aap-1, 0x1.476a9543891bap-3},
    {0x1.b2036576afce6p-1, 0x1.e840b4ac4e4d2p-3},  {0x1.9c2d163a1aa2dp-1, 0x1.40645f0c6651cp-2},
    {0x1.886e6037841edp-1, 0x1.88e9c2c1b9ff8p-2},  {0x1.767dcf5534862p-1, 0x1.ce0a44eb17bccp-2}};

TS_HD float ts_powf(float x, float y) {
  uint32_t ix = as_u32(x);
  if (ix == 0) return 0.0f;                      // +0 ^ (y > 0)
  if (ix == 0x3f800000u) return 1.0f;
  if (ix >= 0x7f800000u) return x + x;           // inf, NaN, negative: outside the callers' domain
  if (ix < 0x00800000u) {                        // subnormal: normalise
    ix = as_u32(x * 0x1p23f) & 0x7fffffffu;
    ix -= 23u << 23;
  }
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (tmp >> 19) % 16;
  const uint32_t top = tmp & 0xff800000u;
  const uint32_t iz = ix - top;
  const int k = (int32_t)top >> 23;
  const double invc = kLog2Tab[i][0], logc = kLog2Tab[i][1];
  const double z = (double)as_f32(iz);
  const double r = z * invc - 1.0;
  const double y0 = logc + (double)k;
  const double r2 = r * r;
  double yy = 0x1.27616c9496e0bp-2 * r + -0x1.71969a075c67ap-2;
  const double p = 0x1.ec70a6ca7baddp-2 * r + -0x1.7154748bef6c8p-1;
  const double r4 = r2 * r2;
  double q = 0x1.71547652ab82bp+0 * r + y0;
  q = p * r2 + q;
  yy = yy * r4 + q;                              // log2(x)
  const double ylogx = (double)y * yy;
  if (((as_u64(ylogx) >> 47) & 0xffff) >= (as_u64(126.0) >> 47)) {  // |y log2 x| >= 126
    if (ylogx > 0x1.fffffffd1d571p+6) return as_f32(0x7f800000u);
    if (ylogx <= -150.0) return 0.0f;
  }
  const double shift = 0x1.8p+47;                // 0x1.8p52 / 32
  double kd = ylogx + shift;
  const uint64_t ki = as_u64(kd);
  kd -= shift;
  const double r1 = ylogx - kd;
  return (float)exp2_tail(ki, r1, 0x1.c6af84b912394p-5, 0x1.ebfce50fac4f3p-3, 0x1.62e42ff0c52d6p-1);
}

// sinf / cosf / sincosf for |x| < 120 (sincosf.h of the same routines): n = round(x / (pi / 2)), the sine or
// the cosine polynomial of the remainder by n's parity, the sign by its bit 1
TS_HD float sincos_poly(double x, double x2, bool neg, bool cosine) {
  if (!cosine) {
    const double s1 = -0x1.555545995a603p-3;  // the sine's coefficients are the same in both tables
    const double s2 = 0x1.1107605230bc4p-7, s3 = -0x1.994eb3774cf24p-13;
    const double x3 = x * x2;
    const double t1 = s2 + x2 * s3;
    const double x7 = x3 * x2;
    const double s = x + x3 * s1;
    return (float)(s + x7 * t1);
  }
  // the second table negates the cosine's coefficients
  const double sg = neg ? -1.0 : 1.0;
  const double c0 = sg * 0x1p0, c1 = sg * -0x1.ffffffd0c621cp-2, c2 = sg * 0x1.55553e1068f19p-5;
  const double c3 = sg * -0x1.6c087e89a359dp-10, c4 = sg * 0x1.99343027bf8c3p-16;
  const double x4 = x2 * x2;
  const double t2 = c3 + x2 * c4;
  const double t1 = c0 + x2 * c1;
  const double x6 = x4 * x2;
  const double c = t1 + x4 * c2;
  return (float)(c + x6 * t2);
}

// which: 0 sine, 1 cosine
TS_HD float ts_sincosf(float y, int which) {
  const uint32_t abstop = (as_u32(y) >> 20) & 0x7ff;
  double x = (double)y;
  if (abstop < 0x3f4) {  // |y| < pi / 4 (top 12 bits of 0x1.921FB6p-1f)
    if (abstop < 0x398) return which ? 1.0f : y;  // |y| < 2^-12
    return sincos_poly(x, x * x, false, which != 0);
  }
  if (abstop >= 0x42f) return y - y;  // |y| >= 120, inf, NaN: outside the callers' domain
  const double r = x * 0x1.45F306DC9C883p+23;
  const int n = ((int32_t)r + 0x800000) >> 24;
  x = x - (double)n * 0x1.921FB54442D18p0;
  const int m = n + which;  // cos(x) = sin(x + pi / 2): the cosine takes the polynomial of the other parity
  // sign[n & 3] = {1, -1, -1, 1} applies to the sine's argument; the cosine polynomials are even
  const double sgn = ((n & 3) == 1 || (n & 3) == 2) ? -1.0 : 1.0;
  return sincos_poly(x * sgn, x * x, (n & 2) != 0, (m & 1) != 0);
}
TS_HD float ts_sinf(float y) { return ts_sincosf(y, 0); }
TS_HD float ts_cosf(float y) { return ts_sincosf(y, 1); }

// fp64 sine and cosine for the Create-time tables (|x| <= pi): Taylor series summed from the small end
TS_HD double ts_sin64(double x) {
  const double x2 = x * x;
  double s = 0.0;
  for (int k = 41; k >= 3; k -= 2) s = (s + 1.0) * (-x2 / (double)(k * (k - 1)));
  return x + x * s;
}
TS_HD double ts_cos64(double x) {
  const double x2 = x * x;
  double s = 0.0;
  for (int k = 40; k >= 2; k -= 2) s = (s + 1.0) * (-x2 / (double)(k * (k - 1)));
  return 1.0 + s;
}

// ------------------------------------------------------------------------------------------- tables
// ns/windows_private.h by formula: kBlocks80w128, kBlocks160w256 and kBlocks320w512 are sin(pi i / (2 r))
// over ramps of r = 3 n / 8 samples around a flat top, printed with eight decimals; kBlocks480w1024 is
// sinf((float)(pi_f k / 960)) for k = i - 32 in 1..959, printed the same way, and zero elsewhere.
inline float decimal8(double s) {
  const double q = (double)(long long)(s * 1e8 + 0.5);
  return (float)(q / 1e8);
}
inline void make_window(int n, float* out) {
  const double pi = 3.14159265358979323846;
  if (n == 1024) {
    for (int i = 0; i < n; ++i) {
      const int k = i - 32;
      if (k < 1 || k > 959) { out[i] = 0.0f; continue; }
      const float arg = (float)((double)kPi * k / 960.0);
      out[i] = decimal8((double)(float)ts_sin64((double)arg));
    }
    return;
  }
  const int r = 3 * n / 8;
  for (int i = 0; i < n; ++i) {
    if (i >= r && i <= n - r) { out[i] = 1.0f; continue; }
    const int k = i < r ? i : n - i;
    out[i] = decimal8(ts_sin64(pi * (double)k / (double)(2 * r)));
  }
}

TS_HD int bit_reverse(int i, int bits) {
  int r = 0;
  for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
  return r;
}
TS_HD int log2i(int v) {
  int b = 0;
  while ((1 << b) < v) ++b;
  return b;
}

// makewt(nw = n / 4) with its bitrv2, then makect(nc = n / 4) behind it (fft4g.c:642-687): n / 2 floats
inline void make_fft_w(int n, float* w) {
  const int nw = n >> 2, nwh = nw >> 1;
  float tmp[kMaxN / 4];
  const float delta = 0.785398185253143310546875f / (float)nwh;  // (float)atan(1.0f) / nwh
  tmp[0] = 1;
  tmp[1] = 0;
  tmp[nwh] = (float)ts_cos64((double)(delta * nwh));
  tmp[nwh + 1] = tmp[nwh];
  for (int j = 2; j < nwh; j += 2) {
    const float x = (float)ts_cos64((double)(delta * j)), y = (float)ts_sin64((double)(delta * j));
    tmp[j] = x;
    tmp[j + 1] = y;
    tmp[nw - j] = y;
    tmp[nw - j + 1] = x;
  }
  const int bits = log2i(nwh);
  for (int j = 0; j < nwh; ++j) {
    const int r = bit_reverse(j, bits);
    w[2 * j] = tmp[2 * r];
    w[2 * j + 1] = tmp[2 * r + 1];
  }
  float* c = w + nw;
  const int nc = nw, nch = nc >> 1;
  c[0] = (float)ts_cos64((double)(delta * nch));
  c[nch] = 0.5f * c[0];
  for (int j = 1; j < nch; ++j) {
    c[j] = 0.5f * (float)ts_cos64((double)(delta * j));
    c[nc - j] = 0.5f * (float)ts_sin64((double)(delta * j));
  }
}

// mean_factor_ (transient_suppressor.cc:143-152)
inline void make_mean_factor(int bins, float* out) {
  for (int i = 0; i < bins; ++i)
    out[i] = 10.f / (1.f + ts_expf(1.f * (float)(i - kMinVoiceBin))) +
             10.f / (1.f + ts_expf(0.3f * (float)(kMaxVoiceBin - i)));
}

TS_HD float phase_of(int r) { return 2 * kPi * (float)r / 32767.f; }
inline void make_phase(float* out) {
  for (int r = 0; r < kPhases; ++r) {
    out[2 * r] = ts_cosf(phase_of(r));
    out[2 * r + 1] = ts_sinf(phase_of(r));
  }
}

// ------------------------------------------------------------------------------------------- configuration
TS_HD bool good_rate(int hz) { return hz == 8000 || hz == 16000 || hz == 32000 || hz == 48000; }

// Initialize's argument checks and lengths; false where it returns -1
TS_HD bool make_config(TsConfig& c, int rate, int det_rate, int channels) {
  if (!good_rate(rate) || !good_rate(det_rate) || channels <= 0) return false;
  c.rate = rate;
  c.det_rate = det_rate;
  c.C = channels;
  c.N = rate == 8000 ? 128 : rate == 16000 ? 256 : rate == 32000 ? 512 : 1024;
  c.L = rate / 100;
  c.delay = c.N - c.L;
  c.bins = c.N / 2 + 1;
  c.D = det_rate / 100;
  c.T = c.D / kLeaves;
  return true;
}

// the state after Initialize; the caller zeroes the stream's buffer array
TS_HD void init_state(AspTsState& s, const TsConfig& c) {
  s.sample_rate_hz = c.rate;
  s.detection_rate_hz = c.det_rate;
  s.num_channels = c.C;
  s.detector_smoothed = 0.f;
  s.keypress_counter = s.chunks_since_keypress = 0;
  s.detection_enabled = s.suppression_enabled = s.use_hard_restoration = 0;
  s.chunks_since_voice_change = 0;
  s.seed = 182;
  s.using_reference = 0;
  s.chunks_at_startup_left_to_delete = 3;
  s.reference_energy = 1.f;
  s.detector_using_reference = 0;
  for (int i = 0; i < 3; ++i) s.previous_results[i] = 0.f;
  for (int i = 0; i < kLeaves; ++i)
    s.last_first_moment[i] = s.last_second_moment[i] = s.moment_sum[i] = s.moment_sum_of_squares[i] = 0.f;
  s.queue_pos = 0;
  for (int i = 0; i < kLeaves; ++i)
    for (int j = 0; j < ASP_TS_MAX_QUEUE; ++j) s.moment_queue[i][j] = 0.f;
  for (int i = 0; i < ASP_TS_NODES; ++i)
    for (int j = 0; j < kHist; ++j) s.node_history[i][j] = 0.f;
}

// ------------------------------------------------------------------------------------------- WebRtc_rdft
// One radix-4 pass at real stride l over n reals: cft1st (l = 2, fft4g.c:1002-1104) and cftmdl (:1107-1231)
// are the same pass over blocks of 4 l reals: block 0 without twiddles, block 1 with w[2] alone, blocks
// 2 u and 2 u + 1 with wk2 = w[2 u], wk1 = w[4 u] or w[4 u + 2], wk3 derived.  The n / 8 butterflies of a
// pass are independent.
TS_HD void cft_pass(int n, int l, float* a, const float* w, const Grp& g) {
  const int half = l >> 1;
  TS_PAR(t, n >> 3) {
    const int B = t / half, j = B * 4 * l + 2 * (t - B * half);
    const int j1 = j + l, j2 = j1 + l, j3 = j2 + l;
    float x0r = a[j] + a[j1], x0i = a[j + 1] + a[j1 + 1];
    const float x1r = a[j] - a[j1], x1i = a[j + 1] - a[j1 + 1];
    const float x2r = a[j2] + a[j3], x2i = a[j2 + 1] + a[j3 + 1];
    const float x3r = a[j2] - a[j3], x3i = a[j2 + 1] - a[j3 + 1];
    a[j] = x0r + x2r;
    a[j + 1] = x0i + x2i;
    if (B == 0) {
      a[j2] = x0r - x2r;
      a[j2 + 1] = x0i - x2i;
      a[j1] = x1r - x3i;
      a[j1 + 1] = x1i + x3r;
      a[j3] = x1r + x3i;
      a[j3 + 1] = x1i - x3r;
    } else if (B == 1) {
      const float wk1r = w[2];
      a[j2] = x2i - x0i;
      a[j2 + 1] = x0r - x2r;
      x0r = x1r - x3i;
      x0i = x1i + x3r;
      a[j1] = wk1r * (x0r - x0i);
      a[j1 + 1] = wk1r * (x0r + x0i);
      x0r = x3i + x1r;
      x0i = x3r - x1i;
      a[j3] = wk1r * (x0i - x0r);
      a[j3 + 1] = wk1r * (x0i + x0r);
    } else {
      const int u = B >> 1;
      const float wk2r = w[2 * u], wk2i = w[2 * u + 1];
      x0r -= x2r;
      x0i -= x2i;
      float wk1r, wk1i, wk3r, wk3i;
      if ((B & 1) == 0) {
        wk1r = w[4 * u];
        wk1i = w[4 * u + 1];
        wk3r = wk1r - 2 * wk2i * wk1i;
        wk3i = 2 * wk2i * wk1r - wk1i;
        a[j2] = wk2r * x0r - wk2i * x0i;
        a[j2 + 1] = wk2r * x0i + wk2i * x0r;
      } else {
        wk1r = w[4 * u + 2];
        wk1i = w[4 * u + 3];
        wk3r = wk1r - 2 * wk2r * wk1i;
        wk3i = 2 * wk2r * wk1r - wk1i;
        a[j2] = -wk2i * x0r - wk2r * x0i;
        a[j2 + 1] = -wk2i * x0i + wk2r * x0r;
      }
      x0r = x1r - x3i;
      x0i = x1i + x3r;
      a[j1] = wk1r * x0r - wk1i * x0i;
      a[j1 + 1] = wk1r * x0i + wk1i * x0r;
      x0r = x1r + x3i;
      x0i = x1i - x3r;
      a[j3] = wk3r * x0r - wk3i * x0i;
      a[j3 + 1] = wk3r * x0i + wk3i * x0r;
    }
  }
  grp_sync(g);
}

// bitrv2: the bit reversal of the n / 2 complex points
TS_HD void bit_reverse_points(int n, float* a, const Grp& g) {
  const int m = n >> 1, bits = log2i(m);
  TS_PAR(i, m) {
    const int r = bit_reverse(i, bits);
    if (i < r) {
      const float xr = a[2 * i], xi = a[2 * i + 1];
      a[2 * i] = a[2 * r];
      a[2 * i + 1] = a[2 * r + 1];
      a[2 * r] = xr;
      a[2 * r + 1] = xi;
    }
  }
  grp_sync(g);
}

// cftfsub (back = false, fft4g.c:902-949) and cftbsub (:952-999)
TS_HD void cft_sub(int n, float* a, const float* w, bool back, const Grp& g) {
  cft_pass(n, 2, a, w, g);
  int l = 8;
  while ((l << 2) < n) {
    cft_pass(n, l, a, w, g);
    l <<= 2;
  }
  if ((l << 2) == n) {
    TS_PAR(t, l >> 1) {
      const int j = 2 * t, j1 = j + l, j2 = j1 + l, j3 = j2 + l;
      const float x0r = a[j] + a[j1], x1r = a[j] - a[j1];
      const float x0i = back ? -a[j + 1] - a[j1 + 1] : a[j + 1] + a[j1 + 1];
      const float x1i = back ? -a[j + 1] + a[j1 + 1] : a[j + 1] - a[j1 + 1];
      const float x2r = a[j2] + a[j3], x2i = a[j2 + 1] + a[j3 + 1];
      const float x3r = a[j2] - a[j3], x3i = a[j2 + 1] - a[j3 + 1];
      a[j] = x0r + x2r;
      a[j2] = x0r - x2r;
      a[j1] = x1r - x3i;
      a[j3] = x1r + x3i;
      if (back) {
        a[j + 1] = x0i - x2i;
        a[j2 + 1] = x0i + x2i;
        a[j1 + 1] = x1i - x3r;
        a[j3 + 1] = x1i + x3r;
      } else {
        a[j + 1] = x0i + x2i;
        a[j2 + 1] = x0i - x2i;
        a[j1 + 1] = x1i + x3r;
        a[j3 + 1] = x1i - x3r;
      }
    }
  } else {
    TS_PAR(t, l >> 1) {
      const int j = 2 * t, j1 = j + l;
      const float x0r = a[j] - a[j1];
      const float x0i = back ? -a[j + 1] + a[j1 + 1] : a[j + 1] - a[j1 + 1];
      a[j] += a[j1];
      a[j + 1] = back ? -a[j + 1] - a[j1 + 1] : a[j + 1] + a[j1 + 1];
      a[j1] = x0r;
      a[j1 + 1] = x0i;
    }
  }
  grp_sync(g);
}

// WebRtc_rdft(n, isgn, a, ip, w) with the tables made (fft4g.c:324-361, rftfsub :1234, rftbsub :1259)
TS_HD void rdft(int n, int isgn, float* a, const float* w, const Grp& g) {
  const int m = n >> 1, nc = n >> 2;
  const float* c = w + (n >> 2);
  if (isgn >= 0) {
    bit_reverse_points(n, a, g);
    cft_sub(n, a, w, false, g);
    TS_PAR(t, (m >> 1) - 1) {
      const int j = 2 * (t + 1), k = n - j, kk = t + 1;
      const float wkr = 0.5f - c[nc - kk], wki = c[kk];
      const float xr = a[j] - a[k], xi = a[j + 1] + a[k + 1];
      const float yr = wkr * xr - wki * xi, yi = wkr * xi + wki * xr;
      a[j] -= yr;
      a[j + 1] -= yi;
      a[k] += yr;
      a[k + 1] -= yi;
    }
    if (g.lane == 0) {
      const float xi = a[0] - a[1];
      a[0] += a[1];
      a[1] = xi;
    }
    grp_sync(g);
  } else {
    if (g.lane == 0) {
      a[1] = 0.5f * (a[0] - a[1]);
      a[0] -= a[1];
      a[1] = -a[1];
      a[m + 1] = -a[m + 1];
    }
    TS_PAR(t, (m >> 1) - 1) {
      const int j = 2 * (t + 1), k = n - j, kk = t + 1;
      const float wkr = 0.5f - c[nc - kk], wki = c[kk];
      const float xr = a[j] - a[k], xi = a[j + 1] + a[k + 1];
      const float yr = wkr * xr + wki * xi, yi = wkr * xi - wki * xr;
      a[j] -= yr;
      a[j + 1] = yi - a[j + 1];
      a[k] += yr;
      a[k + 1] = yi - a[k + 1];
    }
    grp_sync(g);
    bit_reverse_points(n, a, g);
    cft_sub(n, a, w, true, g);
  }
}

// ------------------------------------------------------------------------------------------- detector
// The Daubechies wavelet with 8 vanishing moments (db8), decomposition low-pass filter, 16 taps, written from
// the published filter (the values PyWavelets lists as db8.dec_lo); rounded to float they are the reference's
// kDaubechies8LowPassCoefficients.  The high-pass filter is its mirror with alternating signs.
static constexpr float kDb8Low[kTaps] = {
    -0.00011747678400228192f, 0.00067544940599855677f, -0.00039174037299597711f, -0.0048703529930106603f,
    0.0087460940470156547f, 0.013981027917015516f, -0.044088253931064719f, -0.017369301002022108f,
    0.12874742662018601f, 0.00047248457399797254f, -0.28401554296242809f, -0.015829105256023893f,
    0.58535468365486909f, 0.67563073629801285f, 0.31287159091446592f, 0.054415842243081609f};

// FIRFilterSSE2's reversed coefficient j of the low-pass (hp = 0) or high-pass (hp = 1) filter
TS_HD float db8_reversed(int hp, int j) {
  // low: coefficients[15 - j]; high[i] = (-1)^(i + 1) low[15 - i], reversed: high[15 - j] = (-1)^j low[j]
  return hp ? ((j & 1) ? -kDb8Low[j] : kDb8Low[j]) : kDb8Low[kTaps - 1 - j];
}

// offsets into TsWork::tree: level 0..2 nodes are [15 history][length], level 3 the bare leaves
TS_HD int tree_node(const TsConfig& c, int level, int k) {
  const int D = c.D;
  if (level == 0) return 0;
  if (level == 1) return (kHist + D) + k * (kHist + D / 2);
  if (level == 2) return (kHist + D) + 2 * kHist + D + k * (kHist + D / 4);
  return (kHist + D) + 2 * kHist + D + 4 * kHist + D + k * (D / 8);
}

// WebRtcSpl_RandU's recurrence, k steps at once: seed_k = A^k seed + (A^k - 1) / (A - 1) mod 2^31
TS_HD uint32_t lcg_jump(uint32_t seed, uint32_t k) {
  uint32_t acc_a = 1, acc_c = 0, cur_a = 69069u, cur_c = 1;
  while (k) {
    if (k & 1) {
      acc_a *= cur_a;
      acc_c = acc_c * cur_a + cur_c;
    }
    cur_c = (cur_a + 1) * cur_c;
    cur_a *= cur_a;
    k >>= 1;
  }
  return (acc_a * seed + acc_c) & 0x7fffffffu;
}

// TransientDetector::Detect (transient_detector.cc:69-139) without its last line; the result is left in
// w.scal[0] on lane 0's behalf and the caller syncs
TS_HD void detect(const TsConfig& c, AspTsState& st, TsWork& w, const float* det, const float* ref, int ref_len,
                  const Grp& g) {
  const int D = c.D, T = c.T;
  float* tree = w.tree;
  // ReferenceDetectionValue's energy (:154-156): the reference chunk goes through LDS in pieces, lanes on
  // consecutive samples, and lane 0 adds the squares in the reference's order
  if (ref) {
    if (g.lane == 0) w.scal[2] = 0.f;
    for (int base = 1; base < ref_len; base += kMaxDet) {
      const int n = ref_len - base < kMaxDet ? ref_len - base : kMaxDet;
      TS_PAR(i, n) w.term[i] = ref[base + i];
      grp_sync(g);
      if (g.lane == 0) {
        float energy = w.scal[2];
        for (int i = 0; i < n; ++i) energy += w.term[i] * w.term[i];
        w.scal[2] = energy;
      }
      grp_sync(g);
    }
  }
  // WPDTree::Update: the root takes the data; every node's children filter its [history][data]
  TS_PAR(i, D) tree[kHist + i] = det[i];
  TS_PAR(i, ASP_TS_NODES * kHist) {
    const int node = i / kHist, j = i - node * kHist;
    const int level = node == 0 ? 0 : node < 3 ? 1 : 2, k = node - ((1 << level) - 1);
    tree[tree_node(c, level, k) + j] = st.node_history[node][j];
  }
  grp_sync(g);
  for (int level = 0; level < 3; ++level) {
    const int clen = D >> (level + 1);  // a child's length
    TS_PAR(t, D) {
      const int child = t / clen, k = t - child * clen;
      const float* s = tree + tree_node(c, level, child >> 1) + (2 * k + 1);  // state_[i .. i + 15], i odd
      const int hp = child & 1;
      float l[4];
      for (int m = 0; m < 4; ++m) {
        float acc = 0.f;
        for (int q = 0; q < 4; ++q) acc = acc + s[m + 4 * q] * db8_reversed(hp, m + 4 * q);
        l[m] = acc;
      }
      const float v = (l[0] + l[2]) + (l[1] + l[3]);
      tree[tree_node(c, level + 1, child) + (level < 2 ? kHist : 0) + k] = ts_fabsf(v);
    }
    grp_sync(g);
  }
  TS_PAR(i, ASP_TS_NODES * kHist) {
    const int node = i / kHist, j = i - node * kHist;
    const int level = node == 0 ? 0 : node < 3 ? 1 : 2, k = node - ((1 << level) - 1);
    st.node_history[node][j] = tree[tree_node(c, level, k) + (D >> level) + j];
  }
  // MovingMoments::CalculateMoments, one leaf per lane; the queue of 3 T entries is a ring of three chunks
  TS_PAR(leaf, kLeaves) {
    const float* x = tree + tree_node(c, 3, leaf);
    float* q = st.moment_queue[leaf] + st.queue_pos * T;
    float sum = st.moment_sum[leaf], sq = st.moment_sum_of_squares[leaf];
    const float len = (float)(3 * T);
    for (int j = 0; j < T; ++j) {
      const float old = q[j], v = x[j];
      q[j] = v;
      sum += v - old;
      sq += v * v - old * old;
      w.m1[leaf][j] = sum / len;
      w.m2[leaf][j] = sq / len;
    }
    st.moment_sum[leaf] = sum;
    st.moment_sum_of_squares[leaf] = sq;
  }
  grp_sync(g);
  TS_PAR(t, kLeaves * T) {
    const int leaf = t / T, j = t - leaf * T;
    const float x = tree[tree_node(c, 3, leaf) + j];
    const float first = j ? w.m1[leaf][j - 1] : st.last_first_moment[leaf];
    const float second = j ? w.m2[leaf][j - 1] : st.last_second_moment[leaf];
    const float unbiased = x - first;
    w.term[t] = unbiased * unbiased / (second + FLT_MIN);
  }
  grp_sync(g);
  if (g.lane == 0) {
    float result = 0.f;
    for (int t = 0; t < kLeaves * T; ++t) result += w.term[t];
    for (int leaf = 0; leaf < kLeaves; ++leaf) {
      st.last_first_moment[leaf] = w.m1[leaf][T - 1];
      st.last_second_moment[leaf] = w.m2[leaf][T - 1];
    }
    st.queue_pos = st.queue_pos == 2 ? 0 : st.queue_pos + 1;
    result /= (float)T;
    // ReferenceDetectionValue (:144-171)
    float factor = 1.f;
    st.detector_using_reference = 0;
    if (ref) {
      const float energy = w.scal[2];
      if (energy != 0.f) {
        factor = 1.f / (1.f + ts_expf(20.f * (0.2f - energy / st.reference_energy)));
        st.reference_energy = 0.99f * st.reference_energy + (1.f - 0.99f) * energy;
        st.detector_using_reference = 1;
      }
    }
    result *= factor;
    if (st.chunks_at_startup_left_to_delete > 0) {
      st.chunks_at_startup_left_to_delete--;
      result = 0.f;
    }
    if (result >= 16.f) {
      result = 1.f;
    } else {
      const float horizontal_scaling = kPi / 16.f;
      result = (ts_cosf(result * horizontal_scaling + kPi) + 1.f) * 0.5f;
      result *= result;
    }
    st.previous_results[0] = st.previous_results[1];
    st.previous_results[1] = st.previous_results[2];
    st.previous_results[2] = result;
    float best = st.previous_results[0];
    if (best < st.previous_results[1]) best = st.previous_results[1];
    if (best < st.previous_results[2]) best = st.previous_results[2];
    w.scal[0] = best;
  }
}

// ------------------------------------------------------------------------------------------- suppressor
TS_HD void update_keypress(AspTsState& s, bool key_pressed) {  // transient_suppressor.cc:284-313
  if (key_pressed) {
    s.keypress_counter += 100;
    s.chunks_since_keypress = 0;
    s.detection_enabled = 1;
  }
  s.keypress_counter = s.keypress_counter - 1 > 0 ? s.keypress_counter - 1 : 0;
  if (s.keypress_counter > 100) {
    s.suppression_enabled = 1;
    s.keypress_counter = 0;
  }
  if (s.detection_enabled && ++s.chunks_since_keypress > 400) {
    s.detection_enabled = 0;
    s.suppression_enabled = 0;
    s.keypress_counter = 0;
  }
}

TS_HD void update_restoration(AspTsState& s, float voice_probability) {  // :315-334
  const int not_voiced = voice_probability < 0.02f;
  if (not_voiced == s.use_hard_restoration) {
    s.chunks_since_voice_change = 0;
  } else {
    ++s.chunks_since_voice_change;
    if ((s.use_hard_restoration && s.chunks_since_voice_change > 3) ||
        (!s.use_hard_restoration && s.chunks_since_voice_change > 80)) {
      s.use_hard_restoration = not_voiced;
      s.chunks_since_voice_change = 0;
    }
  }
}

// HardRestoration (:369-389).  The seed advances once per bin that passes the condition, in bin order: each
// lane counts the passing bins of its slice, lane 0 scans the 64 counts, and every lane jumps the LCG ahead
// to its slice's first draw.
TS_HD void hard_restoration(const TsConfig& c, const TsTables& tb, AspTsState& st, TsWork& w, const float* mean,
                            const Grp& g) {
  float* fb = w.s.fb;
  const int slice = (c.bins + 63) / 64;
  TS_PAR(k, 64) {
    int n = 0;
    for (int i = k * slice; i < (k + 1) * slice && i < c.bins; ++i) n += (w.mag[i] > mean[i] && w.mag[i] > 0) ? 1 : 0;
    w.cnt[k] = n;
  }
  grp_sync(g);
  if (g.lane == 0) {
    int run = 0;
    for (int k = 0; k < 64; ++k) {
      const int n = w.cnt[k];
      w.cnt[k] = run;
      run += n;
    }
    w.cnt[64] = run;
  }
  grp_sync(g);
  const float detector_result = 1.f - ts_powf(1.f - st.detector_smoothed, st.using_reference ? 200.f : 50.f);
  const uint32_t seed0 = st.seed;
  TS_PAR(k, 64) {
    uint32_t seed = lcg_jump(seed0, (uint32_t)w.cnt[k]);
    for (int i = k * slice; i < (k + 1) * slice && i < c.bins; ++i) {
      const float m = w.mag[i], sm = mean[i];
      if (m > sm && m > 0) {
        seed = (seed * 69069u + 1u) & 0x7fffffffu;
        const int r = (int)(seed >> 16);
        const float scaled_mean = detector_result * sm;
        fb[2 * i] = (1 - detector_result) * fb[2 * i] + scaled_mean * tb.phase[2 * r];
        fb[2 * i + 1] = (1 - detector_result) * fb[2 * i + 1] + scaled_mean * tb.phase[2 * r + 1];
        w.mag[i] = m - detector_result * (m - sm);
      }
    }
  }
  grp_sync(g);
  if (g.lane == 0) st.seed = lcg_jump(seed0, (uint32_t)w.cnt[64]);
  grp_sync(g);
}

// SoftRestoration (:396-422)
TS_HD void soft_restoration(const TsConfig& c, const TsTables& tb, const AspTsState& st, TsWork& w, const float* mean,
                            const Grp& g) {
  float* fb = w.s.fb;
  if (g.lane == 0) {
    float block_frequency_mean = 0;
    for (int i = kMinVoiceBin; i < kMaxVoiceBin; ++i) block_frequency_mean += w.mag[i];
    w.scal[1] = block_frequency_mean / (float)(kMaxVoiceBin - kMinVoiceBin);
  }
  grp_sync(g);
  const float block_frequency_mean = w.scal[1];
  TS_PAR(i, c.bins) {
    const float m = w.mag[i], sm = mean[i];
    if (m > sm && m > 0 && (st.using_reference || m < block_frequency_mean * tb.mean_factor[i])) {
      const float new_magnitude = m - st.detector_smoothed * (m - sm);
      const float magnitude_ratio = new_magnitude / m;
      fb[2 * i] *= magnitude_ratio;
      fb[2 * i + 1] *= magnitude_ratio;
      w.mag[i] = new_magnitude;
    }
  }
  grp_sync(g);
}

// TransientSuppressor::Suppress on one chunk of one stream (:165-282).  st and w are the group's (LDS on the
// device); in / out / mean are the stream's buffers, data its [C][L] chunk, det its detection chunk (the
// caller passes data where the reference falls back to in_buffer_[buffer_delay_]).  Returns 0, or -1 with
// nothing touched.
TS_HD int suppress_chunk(const TsConfig& c, const TsTables& tb, AspTsState& st, TsWork& w, float* in, float* out,
                         float* mean, float* data, const float* det, const float* ref, int ref_len,
                         float voice_probability, int key_pressed, const Grp& g) {
  if (voice_probability < 0 || voice_probability > 1) return -1;
  const int N = c.N, L = c.L, delay = c.delay;
  if (g.lane == 0) {
    update_keypress(st, key_pressed != 0);
    if (st.detection_enabled) update_restoration(st, voice_probability);
  }
  grp_sync(g);
  if (st.detection_enabled) {
    detect(c, st, w, det, ref, ref_len, g);
    if (g.lane == 0) {
      const float detector_result = w.scal[0];
      st.using_reference = st.detector_using_reference;
      const float smooth_factor = st.using_reference ? 0.6 : 0.1;
      st.detector_smoothed = detector_result >= st.detector_smoothed
                                 ? detector_result
                                 : smooth_factor * st.detector_smoothed + (1 - smooth_factor) * detector_result;
    }
    grp_sync(g);
  }
  float* fb = w.s.fb;
  float* xb = w.s.xb;
  const float fft_scaling = 2.f / (float)N;
  for (int ch = 0; ch < c.C; ++ch) {
    float* in_c = in + (size_t)ch * N;
    float* out_c = out + (size_t)ch * N;
    float* mean_c = mean + (size_t)ch * c.bins;
    float* data_c = data + (size_t)ch * L;
    // UpdateBuffers: the shifted in_buffer_ with the new chunk behind it, staged so that no lane reads what
    // another has already overwritten
    TS_PAR(i, N) xb[i] = i < delay ? in_c[i + L] : data_c[i - delay];
    grp_sync(g);
    TS_PAR(i, N) in_c[i] = xb[i];
    if (!st.suppression_enabled) TS_PAR(i, L) data_c[i] = xb[i];
    if (!st.detection_enabled) {
      grp_sync(g);
      continue;
    }
    TS_PAR(i, N) fb[i] = xb[i] * tb.window[i];
    grp_sync(g);
    rdft(N, 1, fb, tb.w, g);
    if (g.lane == 0) {
      fb[N] = fb[1];
      fb[N + 1] = 0.f;
      fb[1] = 0.f;
    }
    grp_sync(g);
    TS_PAR(i, c.bins) w.mag[i] = ts_fabsf(fb[2 * i]) + ts_fabsf(fb[2 * i + 1]);
    grp_sync(g);
    if (st.suppression_enabled) {
      if (st.use_hard_restoration)
        hard_restoration(c, tb, st, w, mean_c, g);
      else
        soft_restoration(c, tb, st, w, mean_c, g);
    }
    TS_PAR(i, c.bins) mean_c[i] = (1 - 0.5f) * mean_c[i] + 0.5f * w.mag[i];
    if (g.lane == 0) fb[1] = fb[N];
    grp_sync(g);
    rdft(N, -1, fb, tb.w, g);
    // the shifted out_buffer_ (its new chunk zeroed) plus the windowed block
    TS_PAR(i, N) {
      float o = i < delay ? out_c[i + L] : 0.f;
      o += fb[i] * tb.window[i] * fft_scaling;
      xb[i] = o;
    }
    grp_sync(g);
    TS_PAR(i, N) out_c[i] = xb[i];
    if (st.suppression_enabled) TS_PAR(i, L) data_c[i] = xb[i];
    grp_sync(g);
  }
  return 0;
}

}  // namespace aspts
#endif  // ASP_TS_CORE_H_
