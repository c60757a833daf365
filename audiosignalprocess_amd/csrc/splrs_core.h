// splrs_core.h -- one channel of the fixed-point resampler, restated with the reference's integer semantics
// (common_audio/resampler/resampler.cc over resample_by_2.c, resample_48khz.c, resample.c,
// resample_by_2_internal.c and resample_fractional.c).
//
// One source for two builds.  A channel is served by LANES lanes, every loop is written
// "for (i = lane; i < n; i += LANES)":
//   * the two (LPBy2: four, run as two pairs) all-pass branches of a by-2 stage are independent cascades:
//     the loop over branches puts one cascade on a lane, with its four state words in registers;
//   * the fractional FIR stages and the combine steps are independent per output sample;
//   * wsync() orders one lane's stores before another lane's loads (a fence inside the wave);
//   * the kernel (splrs_kernels.hip) runs it with LANES = 16, the CPU build (splrs_restate.cpp) with
//     LANES = 1: plain loops in the reference's order.
// Nothing is re-associated: a cascade is the reference's recurrence, and the FIR sums are wrapping int32
// sums (associative mod 2^32) written in the reference's order anyway.  All recurrences run in wrapping
// 32-bit arithmetic (unsigned where signed would overflow) with truncating shifts; saturation only where
// the reference saturates.
//
// A Push is cut into pieces of one block of the mode's block loop (10 ms; 240 / 480 samples for the modes
// without one).  Every primitive is a streaming filter over its state, so the pieces give what one pass over
// the whole length gives.  A mode is a chain of up to three primitives over state1_ / state2_ / state3_
// (32 words each) that ping-pongs between two int16 buffers; the block resamplers use the reference's own
// tmpmem offsets in one int32 work buffer.
#ifndef ASP_SPLRS_CORE_H_
#define ASP_SPLRS_CORE_H_

#include <stdint.h>

#include "asp_resampler.h"

#if defined(__HIPCC__)
#define SPLRS_HD __host__ __device__
#else
#define SPLRS_HD
#endif

namespace aspsplrs {

constexpr int kModes = 21;        // ResamplerMode: 1To1 ... 11To8
constexpr int kStage = 32;        // words per stage state (the longest reference struct)
constexpr int kStateWords = 96;   // state1_, state2_, state3_
constexpr int kPieceMax = 480;    // samples in either int16 buffer
constexpr int kWork = 496;        // int32 work buffer: tmpmem of Resample48khzTo16khz, the longest

enum Op : int8_t { kNone, kUp2, kDown2, k16To48, k48To16, k22To16, k16To22, k22To8, k8To22 };

// block: the reference's lengthIn % block check (0: any length); outLen = lengthIn * num / den;
// piece: samples per piece; op: the chain
struct Chain {
  int16_t block, num, den, piece;
  int8_t op[3];
};
static constexpr Chain kChain[kModes] = {
    {0, 1, 1, 480, {kNone, kNone, kNone}},         // 1To1
    {0, 2, 1, 240, {kUp2, kNone, kNone}},          // 1To2
    {160, 3, 1, 160, {k16To48, kNone, kNone}},     // 1To3
    {0, 4, 1, 120, {kUp2, kUp2, kNone}},           // 1To4
    {80, 6, 1, 80, {kUp2, k16To48, kNone}},        // 1To6
    {40, 12, 1, 40, {kUp2, kUp2, k16To48}},        // 1To12
    {160, 3, 2, 160, {k16To48, kDown2, kNone}},    // 2To3
    {80, 11, 2, 80, {kUp2, k8To22, kNone}},        // 2To11
    {80, 11, 4, 80, {k8To22, kNone, kNone}},       // 4To11
    {160, 11, 8, 160, {k16To22, kNone, kNone}},    // 8To11
    {110, 16, 11, 110, {kUp2, k22To16, kNone}},    // 11To16
    {110, 32, 11, 110, {kUp2, k22To16, kUp2}},     // 11To32
    {0, 1, 2, 480, {kDown2, kNone, kNone}},        // 2To1
    {480, 1, 3, 480, {k48To16, kNone, kNone}},     // 3To1
    {0, 1, 4, 480, {kDown2, kDown2, kNone}},       // 4To1
    {480, 1, 6, 480, {k48To16, kDown2, kNone}},    // 6To1
    {480, 1, 12, 480, {k48To16, kDown2, kDown2}},  // 12To1
    {240, 2, 3, 240, {kUp2, k48To16, kNone}},      // 3To2 (the reference checks 2 * lengthIn % 480)
    {220, 2, 11, 220, {k22To8, kDown2, kNone}},    // 11To2
    {220, 4, 11, 220, {k22To8, kNone, kNone}},     // 11To4
    {220, 8, 11, 220, {k22To16, kNone, kNone}},    // 11To8
};

// Resampler::Reset's mode table (resampler.cc:162-276): the mode, or -1
SPLRS_HD inline int select_mode(int in_freq, int out_freq) {
  if (in_freq <= 0 || out_freq <= 0) return -1;
  int a = in_freq, b = out_freq, c = a % b;
  while (c != 0) {
    a = b;
    b = c;
    c = a % b;
  }
  const int i = in_freq / b, o = out_freq / b;
  if (i == o) return 0;
  if (i == 1) return o == 2 ? 1 : o == 3 ? 2 : o == 4 ? 3 : o == 6 ? 4 : o == 12 ? 5 : -1;
  if (o == 1) return i == 2 ? 12 : i == 3 ? 13 : i == 4 ? 14 : i == 6 ? 15 : i == 12 ? 16 : -1;
  if (i == 2) return o == 3 ? 6 : o == 11 ? 7 : -1;
  if (i == 4) return o == 11 ? 8 : -1;
  if (i == 8) return o == 11 ? 9 : -1;
  if (i == 3) return o == 2 ? 17 : -1;
  if (i == 11) return o == 2 ? 18 : o == 4 ? 19 : o == 16 ? 10 : o == 32 ? 11 : o == 8 ? 20 : -1;
  return -1;
}

// Push's per-mode checks (resampler.cc:497-994): outLen, or -1
SPLRS_HD inline int check_push(int mode, int length_in, int max_len) {
  if (mode < 0 || mode >= kModes || length_in < 0 || length_in > (1 << 24)) return -1;
  const Chain& c = kChain[mode];
  if (c.block && length_in % c.block) return -1;
  const int out = length_in * c.num / c.den;
  return max_len < out ? -1 : out;
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
#else
SPLRS_HD inline void wsync() {}
#endif

SPLRS_HD inline int32_t wadd(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
SPLRS_HD inline int32_t wsub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
SPLRS_HD inline int32_t wmul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }
SPLRS_HD inline int32_t wshl(int32_t a, int k) { return (int32_t)((uint32_t)a << k); }
SPLRS_HD inline int16_t sat16(int32_t v) { return (int16_t)(v > 32767 ? 32767 : v < -32768 ? -32768 : v); }

// ------------------------------------------------------------------ resample_by_2.c
// WEBRTC_SPL_SCALEDIFF32(A, B, C) with a 16-bit unsigned A
SPLRS_HD inline int32_t scalediff(uint32_t a, int32_t b, int32_t c) {
  return (int32_t)((uint32_t)c + (uint32_t)((b >> 16) * (int32_t)a) + (((uint32_t)(b & 0xFFFF) * a) >> 16));
}

// One sample through a three-section all-pass of resample_by_2.c; k: 0 kResampleAllpass1, 1 kResampleAllpass2
SPLRS_HD inline int32_t ap3q(int32_t x, int k, int32_t (&s)[4]) {
  const uint32_t c0 = k ? 12199 : 3284, c1 = k ? 37471 : 24441, c2 = k ? 60255 : 49528;
  const int32_t t1 = scalediff(c0, wsub(x, s[1]), s[0]);
  s[0] = x;
  const int32_t t2 = scalediff(c1, wsub(t1, s[2]), s[1]);
  s[1] = t1;
  s[3] = scalediff(c2, wsub(t2, s[3]), s[2]);
  s[2] = t2;
  return s[3];
}

// WebRtcSpl_UpsampleBy2: branch 0 (state 0..3, Allpass1) makes the even outputs, branch 1 (4..7, Allpass2) the odd
template <int LANES>
SPLRS_HD inline void upsample_by2(const int16_t* in, int len, int16_t* out, int32_t* st, int lane) {
  for (int br = lane; br < 2; br += LANES) {
    int32_t s[4] = {st[4 * br], st[4 * br + 1], st[4 * br + 2], st[4 * br + 3]};
    for (int i = 0; i < len; ++i) {
      const int32_t v = ap3q(wshl(in[i], 10), br, s);
      out[2 * i + br] = sat16(wadd(v, 512) >> 10);
    }
    for (int j = 0; j < 4; ++j) st[4 * br + j] = s[j];
  }
  wsync();
}

// WebRtcSpl_DownsampleBy2: branch 0 (state 0..3, Allpass2) takes the even inputs, branch 1 (4..7, Allpass1) the odd;
// w holds the two branch outputs until they are added
template <int LANES>
SPLRS_HD inline void downsample_by2(const int16_t* in, int len, int16_t* out, int32_t* st, int32_t* w, int lane) {
  const int n = len >> 1;
  for (int br = lane; br < 2; br += LANES) {
    int32_t s[4] = {st[4 * br], st[4 * br + 1], st[4 * br + 2], st[4 * br + 3]};
    for (int i = 0; i < n; ++i) w[2 * i + br] = ap3q(wshl(in[2 * i + br], 10), 1 - br, s);
    for (int j = 0; j < 4; ++j) st[4 * br + j] = s[j];
  }
  wsync();
  for (int i = lane; i < n; i += LANES) out[i] = sat16(wadd(wadd(w[2 * i], w[2 * i + 1]), 1024) >> 11);
  wsync();
}

// ------------------------------------------------------------------ resample_by_2_internal.c
// One sample through a three-section all-pass; k: the row of kResampleAllpass
SPLRS_HD inline int32_t ap3(int32_t x, int k, int32_t (&s)[4]) {
  const int32_t c0 = k ? 3050 : 821, c1 = k ? 9368 : 6110, c2 = k ? 15063 : 12382;
  int32_t d = wadd(wsub(x, s[1]), 1 << 13) >> 14;
  const int32_t t1 = wadd(s[0], wmul(d, c0));
  s[0] = x;
  d = wsub(t1, s[2]) >> 14;
  if (d < 0) d += 1;
  const int32_t t0 = wadd(s[1], wmul(d, c1));
  s[1] = t1;
  d = wsub(t0, s[3]) >> 14;
  if (d < 0) d += 1;
  s[3] = wadd(s[2], wmul(d, c2));
  s[2] = t0;
  return s[3];
}
SPLRS_HD inline int32_t q15(int16_t x) { return wadd(wshl(x, 15), 1 << 14); }

// WebRtcSpl_UpBy2ShortToInt: branch 0 is the upper filter (row 0, state 4..7, even outputs), branch 1 the lower
template <int LANES>
SPLRS_HD inline void up_by2_short_to_int(const int16_t* in, int len, int32_t* out, int32_t* st, int lane) {
  for (int br = lane; br < 2; br += LANES) {
    int32_t* sp = st + 4 * (1 - br);
    int32_t s[4] = {sp[0], sp[1], sp[2], sp[3]};
    for (int i = 0; i < len; ++i) out[2 * i + br] = ap3(q15(in[i]), br, s) >> 15;
    for (int j = 0; j < 4; ++j) sp[j] = s[j];
  }
  wsync();
}

// WebRtcSpl_UpBy2IntToShort
template <int LANES>
SPLRS_HD inline void up_by2_int_to_short(const int32_t* in, int len, int16_t* out, int32_t* st, int lane) {
  for (int br = lane; br < 2; br += LANES) {
    int32_t* sp = st + 4 * (1 - br);
    int32_t s[4] = {sp[0], sp[1], sp[2], sp[3]};
    for (int i = 0; i < len; ++i) out[2 * i + br] = sat16(ap3(in[i], br, s) >> 15);
    for (int j = 0; j < 4; ++j) sp[j] = s[j];
  }
  wsync();
}

// WebRtcSpl_DownBy2IntToShort (len / 2 even): branch 0 is the lower filter (row 1, state 0..3) on the even
// inputs, branch 1 the upper on the odd ones; `in` is overwritten, as in the reference
template <int LANES>
SPLRS_HD inline void down_by2_int_to_short(int32_t* in, int len, int16_t* out, int32_t* st, int lane) {
  const int n = len >> 1;
  for (int br = lane; br < 2; br += LANES) {
    int32_t* sp = st + 4 * br;
    int32_t s[4] = {sp[0], sp[1], sp[2], sp[3]};
    for (int i = 0; i < n; ++i) in[2 * i + br] = ap3(in[2 * i + br], 1 - br, s) >> 1;
    for (int j = 0; j < 4; ++j) sp[j] = s[j];
  }
  wsync();
  for (int i = lane; i < n; i += LANES) out[i] = sat16(wadd(in[2 * i], in[2 * i + 1]) >> 15);
  wsync();
}

// WebRtcSpl_LPBy2ShortToInt.  Four cascades in two pairs: first the lower filters (state 0..3 on the odd
// inputs delayed by one, its first input being state[12]; state 8..11 on the even inputs), then the upper
// filters (4..7 on the even inputs, 12..15 on the odd), which add to what the first pair left in `out`.
// The pairs run one after the other, so state[12] is read before the last cascade replaces it.
template <int LANES>
SPLRS_HD inline void lp_by2_short_to_int(const int16_t* in, int len, int32_t* out, int32_t* st, int lane) {
  const int n = len >> 1;
  for (int br = lane; br < 2; br += LANES) {
    int32_t* sp = st + 8 * br;
    int32_t s[4] = {sp[0], sp[1], sp[2], sp[3]};
    int32_t x = st[12];
    for (int i = 0; i < n; ++i) {
      if (br) x = q15(in[2 * i]);
      out[2 * i + br] = ap3(x, 1, s) >> 1;
      if (!br) x = q15(in[2 * i + 1]);
    }
    for (int j = 0; j < 4; ++j) sp[j] = s[j];
  }
  wsync();
  for (int br = lane; br < 2; br += LANES) {
    int32_t* sp = st + 4 + 8 * br;
    int32_t s[4] = {sp[0], sp[1], sp[2], sp[3]};
    for (int i = 0; i < n; ++i) out[2 * i + br] = wadd(out[2 * i + br], ap3(q15(in[2 * i + br]), 0, s) >> 1) >> 15;
    for (int j = 0; j < 4; ++j) sp[j] = s[j];
  }
  wsync();
}

// ------------------------------------------------------------------ resample_fractional.c, resample.c
static constexpr int16_t k48To32[2][8] = {{778, -2050, 1087, 23285, 12903, -3783, 441, 222},
                                          {222, 441, -3783, 12903, 23285, 1087, -2050, 778}};
static constexpr int16_t k32To24[3][8] = {{767, -2362, 2434, 24406, 10620, -3838, 721, 90},
                                          {386, -381, -2646, 19062, 19062, -2646, -381, 386},
                                          {90, 721, -3838, 10620, 24406, 2434, -2362, 767}};
static constexpr int16_t k44To32[4][9] = {{117, -669, 2245, -6183, 26267, 13529, -3245, 845, -138},
                                          {-101, 612, -2283, 8532, 29790, -5138, 1789, -524, 91},
                                          {50, -292, 1016, -3064, 32010, 3933, -1147, 315, -53},
                                          {-156, 974, -3863, 18603, 21691, -6246, 2353, -712, 126}};
static constexpr int16_t k32To22[5][9] = {{127, -712, 2359, -6333, 23456, 16775, -3695, 945, -154},
                                          {-39, 230, -830, 2785, 32366, -2324, 760, -218, 38},
                                          {117, -663, 2222, -6133, 26634, 13070, -3174, 831, -137},
                                          {-77, 457, -1677, 5958, 31175, -4136, 1405, -408, 71},
                                          {98, -560, 1900, -5406, 29240, 9423, -2480, 663, -110}};
// per output sample of a block: coefficient row, first input, direction; output 0 copies input 3
static constexpr int8_t k44To32Tap[8][3] = {{0, 3, 0}, {0, 0, 1}, {1, 2, 1}, {2, 3, 1}, {3, 5, 1}, {2, 14, -1}, {1, 15, -1}, {0, 17, -1}};
static constexpr int8_t k32To22Tap[11][3] = {{0, 3, 0},  {0, 0, 1},   {1, 2, 1},   {2, 3, 1},   {3, 5, 1},  {4, 6, 1},
                                             {4, 16, -1}, {3, 17, -1}, {2, 19, -1}, {1, 20, -1}, {0, 22, -1}};

// WebRtcSpl_Resample48khzTo32khz (P = 2, Q = 3) and WebRtcSpl_Resample32khzTo24khz (P = 3, Q = 4): nout output
// samples, `out` below `in` in the same buffer as in the reference.  A round of LANES outputs reads its
// inputs, then writes: the inputs of a later round lie above everything written so far.
template <int LANES, int P, int Q>
SPLRS_HD inline void fir8(const int32_t* in, int32_t* out, int nout, const int16_t (*coef)[8], int lane) {
  for (int base = 0; base < nout; base += LANES) {
    const int o = base + lane;
    int32_t acc = 1 << 14;
    if (o < nout) {
      const int m = o / P, ph = o - m * P;
      const int32_t* x = in + Q * m + ph;
      for (int j = 0; j < 8; ++j) acc = wadd(acc, wmul(coef[ph][j], x[j]));
    }
    wsync();
    if (o < nout) out[o] = acc;
    wsync();
  }
}

// WebRtcSpl_Resample44khzTo32khz (P = 8, Q = 11, k44To32) and WebRtcSpl_32khzTo22khzIntToInt /
// ...IntToShort (P = 11, Q = 16, k32To22): one inner product per output sample, read then written as in fir8
template <int LANES, int P, int Q, bool SHORT>
SPLRS_HD inline void fir9(const int32_t* in, int32_t* out32, int16_t* out16, int nout, const int16_t (*coef)[9],
                          const int8_t (*tap)[3], int lane) {
  for (int base = 0; base < nout; base += LANES) {
    const int o = base + lane;
    int32_t acc = 1 << 14;
    bool copy = false;
    if (o < nout) {
      const int m = o / P, q = o - m * P;
      const int row = tap[q][0], dir = tap[q][2];
      const int32_t* x = in + Q * m + tap[q][1];
      copy = dir == 0;
      if (copy) {
        acc = SHORT ? x[0] : wadd(wshl(x[0], 15), 1 << 14);
      } else {
        for (int j = 0; j < 9; ++j) acc = wadd(acc, wmul(coef[row][j], x[dir * j]));
      }
    }
    wsync();
    if (o < nout) {
      if (SHORT)
        out16[o] = sat16(copy ? acc : acc >> 15);
      else
        out32[o] = acc;
    }
    wsync();
  }
}

// the FIR stage's eight history words: tmp[0 .. 8) <- state, state <- tmp[n .. n + 8)
template <int LANES>
SPLRS_HD inline void swap_history(int32_t* tmp, int n, int32_t* st, int lane) {
  for (int i = lane; i < 8; i += LANES) {
    tmp[i] = st[i];
    st[i] = tmp[n + i];
  }
  wsync();
}

// ------------------------------------------------------------------ resample_48khz.c, resample.c: the block resamplers
// WebRtcSpl_Resample16khzTo48khz: 160 -> 480; st: S_16_32, S_32_24, S_24_48
template <int LANES>
SPLRS_HD inline void r16to48(const int16_t* in, int16_t* out, int32_t* st, int32_t* w, int lane) {
  up_by2_short_to_int<LANES>(in, 160, w + 16, st, lane);
  swap_history<LANES>(w + 8, 320, st + 8, lane);
  fir8<LANES, 3, 4>(w + 8, w, 240, k32To24, lane);
  up_by2_int_to_short<LANES>(w, 240, out, st + 16, lane);
}

// WebRtcSpl_Resample48khzTo16khz: 480 -> 160; st: S_48_48[16], S_48_32, S_32_16
template <int LANES>
SPLRS_HD inline void r48to16(const int16_t* in, int16_t* out, int32_t* st, int32_t* w, int lane) {
  lp_by2_short_to_int<LANES>(in, 480, w + 16, st, lane);
  swap_history<LANES>(w + 8, 480, st + 16, lane);
  fir8<LANES, 2, 3>(w + 8, w, 320, k48To32, lane);
  down_by2_int_to_short<LANES>(w, 320, out, st + 24, lane);
}

// WebRtcSpl_Resample22khzTo16khz: 220 -> 160 in five sub-blocks; st: S_22_44, S_44_32, S_32_16
template <int LANES>
SPLRS_HD inline void r22to16(const int16_t* in, int16_t* out, int32_t* st, int32_t* w, int lane) {
  for (int k = 0; k < 5; ++k) {
    up_by2_short_to_int<LANES>(in + 44 * k, 44, w + 16, st, lane);
    swap_history<LANES>(w + 8, 88, st + 8, lane);
    fir9<LANES, 8, 11, false>(w + 8, w, nullptr, 64, k44To32, k44To32Tap, lane);
    down_by2_int_to_short<LANES>(w, 64, out + 32 * k, st + 16, lane);
  }
}

// WebRtcSpl_Resample16khzTo22khz: 160 -> 220 in four sub-blocks; st: S_16_32, S_32_22
template <int LANES>
SPLRS_HD inline void r16to22(const int16_t* in, int16_t* out, int32_t* st, int32_t* w, int lane) {
  for (int k = 0; k < 4; ++k) {
    up_by2_short_to_int<LANES>(in + 40 * k, 40, w + 8, st, lane);
    swap_history<LANES>(w, 80, st + 8, lane);
    fir9<LANES, 11, 16, true>(w, nullptr, out + 55 * k, 55, k32To22, k32To22Tap, lane);
  }
}

// WebRtcSpl_Resample22khzTo8khz: 220 -> 80 in two sub-blocks; st: S_22_22[16], S_22_16, S_16_8
template <int LANES>
SPLRS_HD inline void r22to8(const int16_t* in, int16_t* out, int32_t* st, int32_t* w, int lane) {
  for (int k = 0; k < 2; ++k) {
    lp_by2_short_to_int<LANES>(in + 110 * k, 110, w + 16, st, lane);
    swap_history<LANES>(w + 8, 110, st + 16, lane);
    fir9<LANES, 8, 11, false>(w + 8, w, nullptr, 80, k44To32, k44To32Tap, lane);
    down_by2_int_to_short<LANES>(w, 80, out + 40 * k, st + 24, lane);
  }
}

// WebRtcSpl_Resample8khzTo22khz: 80 -> 220 in two sub-blocks; st: S_8_16, S_16_11, S_11_22
template <int LANES>
SPLRS_HD inline void r8to22(const int16_t* in, int16_t* out, int32_t* st, int32_t* w, int lane) {
  for (int k = 0; k < 2; ++k) {
    up_by2_short_to_int<LANES>(in + 40 * k, 40, w + 18, st, lane);
    swap_history<LANES>(w + 10, 80, st + 8, lane);
    fir9<LANES, 11, 16, false>(w + 10, w, nullptr, 55, k32To22, k32To22Tap, lane);
    up_by2_int_to_short<LANES>(w, 55, out + 110 * k, st + 16, lane);
  }
}

// ------------------------------------------------------------------ one piece of a Push
// n samples in a (n: the mode's piece, or what is left of a mode without a block loop) through the mode's
// chain; a and b hold kPieceMax samples each, w kWork words, st kStateWords.  Returns the output count and
// the buffer that holds it.
template <int LANES>
SPLRS_HD inline int push_piece(int mode, int32_t* st, int16_t* a, int n, int16_t* b, int32_t* w, int lane,
                               int16_t** result) {
  const Chain& c = kChain[mode];
  int16_t *src = a, *dst = b;
  for (int k = 0; k < 3 && c.op[k] != kNone; ++k) {
    int32_t* s = st + kStage * k;
    switch (c.op[k]) {
      case kUp2:
        upsample_by2<LANES>(src, n, dst, s, lane);
        n *= 2;
        break;
      case kDown2:
        downsample_by2<LANES>(src, n, dst, s, w, lane);
        n >>= 1;
        break;
      case k16To48:
        r16to48<LANES>(src, dst, s, w, lane);
        n = 480;
        break;
      case k48To16:
        r48to16<LANES>(src, dst, s, w, lane);
        n = 160;
        break;
      case k22To16:
        r22to16<LANES>(src, dst, s, w, lane);
        n = 160;
        break;
      case k16To22:
        r16to22<LANES>(src, dst, s, w, lane);
        n = 220;
        break;
      case k22To8:
        r22to8<LANES>(src, dst, s, w, lane);
        n = 80;
        break;
      case k8To22:   // 2To11 comes here with two blocks
        for (int r = 0; r < n / 80; ++r) r8to22<LANES>(src + 80 * r, dst + 220 * r, s, w, lane);
        n = n / 80 * 220;
        break;
      default:
        break;
    }
    int16_t* t = src;
    src = dst;
    dst = t;
  }
  *result = src;
  return n;
}

}  // namespace aspsplrs
#endif  // ASP_SPLRS_CORE_H_
