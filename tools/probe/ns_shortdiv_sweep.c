/* Envelope sweeps for the short division / square-root chains of ns_device.h (fdiv_c, fdiv_1c, fsqrt_n_wave), on the
 * CPU: for every argument of a call site whose quotient has ONE free float, is a chain with fewer steps than fdiv's
 * seven still the correctly rounded quotient -- whatever the reciprocal instruction returns within an ulp?
 *
 *   gcc -O2 -march=native -ffp-contract=off -fopenmp tools/probe/ns_shortdiv_sweep.c -lm -o ns_shortdiv_sweep
 *   ./ns_shortdiv_sweep            (all four sweeps; profiles/r16_ns_shortdiv_sweep.txt is its output)
 *
 * Every step is one IEEE single operation (fmaf is the hardware's fused multiply-add, nothing else is contracted).
 * The reference quotient is (float)((double)n / (double)d): the double quotient of two floats rounds to the correctly
 * rounded float quotient (53 >= 2 * 24 + 2).  The seed of a chain is RN(1 / d) moved by -1, 0 and +1 ulp: every value
 * an instruction with an error of at most one ulp can return; a form that is right for all three is right on any such
 * hardware, a form that is wrong for some may still be right for the one fixed function a device implements -- that
 * is decided by a sweep on the device (AspNs_debug_compare, function 26).
 *
 *   7-step: r1 = r0 + r0 (1 - d r0); q0 = n r1; q1 = q0 + r1 (n - d q0); q = q1 + r1 (n - d q1)        (fdiv)
 *   S1:     the same without the last correction (q1)                                                  (fdiv_1c)
 *   S2:     the same without the refinement, the seed r0 in both corrections                           (fdiv_c)
 *   S3:     both removed
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static inline float as_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t as_u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float ulp_move(float r, int k) { return as_f(as_u(r) + (uint32_t)k); }  /* r > 0 */

typedef struct { float q7, s1, s2, s3; } Quot;
static inline Quot chains(float n, float d, float r0) {
  Quot o;
  const float r1 = fmaf(fmaf(-d, r0, 1.0f), r0, r0);
  float q0 = n * r1;
  o.s1 = fmaf(fmaf(-d, q0, n), r1, q0);
  o.q7 = fmaf(fmaf(-d, o.s1, n), r1, o.s1);
  q0 = n * r0;
  o.s3 = fmaf(fmaf(-d, q0, n), r0, q0);
  o.s2 = fmaf(fmaf(-d, o.s3, n), r0, o.s3);
  return o;
}
static inline int ne(float a, float b) { return as_u(a) != as_u(b); }

/* 40 / d, every finite float d in [1, 2^127): the quantile trackers' FACTOR / max(density, 1) */
static void sweep_fdiv40(void) {
  unsigned long long cases = 0, w7 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma omp parallel for reduction(+ : cases, w7, w1, w2, w3) schedule(dynamic, 1 << 16)
  for (uint32_t u = 0x3f800000u; u < 0x7f000000u; ++u) {
    const float d = as_f(u), want = (float)(40.0 / (double)d), rn = (float)(1.0 / (double)d);
    for (int k = -1; k <= 1; ++k) {
      const Quot o = chains(40.0f, d, ulp_move(rn, k));
      ++cases; w7 += ne(o.q7, want); w1 += ne(o.s1, want); w2 += ne(o.s2, want); w3 += ne(o.s3, want);
    }
  }
  printf("40 / d, d in [1, 2^127): %llu cases; wrong: 7-step %llu, S1 %llu, S2 %llu, S3 %llu\n", cases, w7, w1, w2, w3);
}

/* (1 - p) / (p + 0.0001f), every float p in [0.01, 1]: gainPrior behind ns_prior_update's clamps */
static void sweep_gainprior(void) {
  unsigned long long cases = 0, w7 = 0, w1 = 0, w2 = 0, w3 = 0;
  const uint32_t lo = as_u(0.01f), hi = as_u(1.0f);
#pragma omp parallel for reduction(+ : cases, w7, w1, w2, w3) schedule(dynamic, 1 << 16)
  for (uint32_t u = lo; u <= hi; ++u) {
    const float p = as_f(u), n = 1.0f - p, d = p + 0.0001f;
    const float want = (float)((double)n / (double)d), rn = (float)(1.0 / (double)d);
    for (int k = -1; k <= 1; ++k) {
      const Quot o = chains(n, d, ulp_move(rn, k));
      ++cases; w7 += ne(o.q7, want); w1 += ne(o.s1, want); w2 += ne(o.s2, want); w3 += ne(o.s3, want);
    }
  }
  printf("(1 - p) / (p + 0.0001f), p in [0.01, 1]: %llu cases; wrong: 7-step %llu, S1 %llu, S2 %llu, S3 %llu\n", cases,
         w7, w1, w2, w3);
}

/* tn / ((1 + tn) + 0.0001f), tn = 2 x, every float x in [0, 2^126): the likelihood ratio's quotient; against the 7-step
 * form (whose own differences from the rounded quotient are counted beside it) */
static void sweep_phase8(void) {
  unsigned long long cases = 0, w7 = 0, d1 = 0, d2 = 0, d1sub = 0;
#pragma omp parallel for reduction(+ : cases, w7, d1, d2, d1sub) schedule(dynamic, 1 << 16)
  for (uint32_t u = 0; u < 0x7e800000u; ++u) {
    const float x = as_f(u), tn = 2.0f * x, t1 = 1.0f + tn, d = t1 + 0.0001f;
    const float want = (float)((double)tn / (double)d), rn = (float)(1.0 / (double)d);
    for (int k = -1; k <= 1; ++k) {
      const Quot o = chains(tn, d, ulp_move(rn, k));
      ++cases; w7 += ne(o.q7, want);
      const int a = ne(o.s1, o.q7);
      d1 += a; d2 += ne(o.s2, o.q7);
      d1sub += a && (tn < 0x1p-126f || want < 0x1p-126f);
    }
  }
  printf("tn / ((1 + tn) + 0.0001f), tn = 2 x, x in [0, 2^126): %llu cases; 7-step wrong %llu; differ from the 7-step "
         "form: S1 %llu (%llu of them with a subnormal numerator or quotient), S2 %llu\n", cases, w7, d1, d1sub, d2);
}

/* sqrt(x), every float x in [2^-100, 2^127): fsqrt's chain, the chain without its e step (g and h unrefined: one
 * correction of x r) and the chain with only h unrefined; the seed is RN(1 / sqrt(x)) moved by -1, 0, +1 ulp */
static void sweep_sqrt(void) {
  unsigned long long cases = 0, w8 = 0, wno_e = 0, wh = 0;
#pragma omp parallel for reduction(+ : cases, w8, wno_e, wh) schedule(dynamic, 1 << 16)
  for (uint32_t u = 0x0d800000u; u < 0x7f000000u; ++u) {
    const float x = as_f(u), want = sqrtf(x), rn = (float)(1.0 / sqrt((double)x));
    for (int k = -1; k <= 1; ++k) {
      const float r = ulp_move(rn, k);
      const float g0 = x * r, h0 = 0.5f * r, e = fmaf(-h0, g0, 0.5f);
      const float g1 = fmaf(g0, e, g0), h1 = fmaf(h0, e, h0);
      const float full = fmaf(fmaf(-g1, g1, x), h1, g1);
      const float href = fmaf(fmaf(-g1, g1, x), h0, g1);
      const float no_e = fmaf(fmaf(-g0, g0, x), h0, g0);
      ++cases; w8 += ne(full, want); wno_e += ne(no_e, want); wh += ne(href, want);
    }
  }
  printf("sqrt(x), x in [2^-100, 2^127): %llu cases; wrong: full chain %llu, without the e step %llu, h unrefined %llu\n",
         cases, w8, wno_e, wh);
}

int main(void) {
  sweep_fdiv40();
  sweep_gainprior();
  sweep_phase8();
  sweep_sqrt();
  return 0;
}
