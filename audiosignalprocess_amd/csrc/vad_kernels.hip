// vad_kernels.hip -- the batched voice activity detector on gfx950 (include/asp_vad.h).
//
// One lane per stream, one wave per workgroup.  A call of F frames loads each lane's
// VadInstT once into registers (filter states, GMM tables, thresholds) and LDS (the 2 x 96 FindMinimum
// vectors, [k][lane] so that a wave's accesses fall on consecutive banks), runs the frames in time order
// and stores the state once.  Input is staged 10 ms at a time through LDS with coalesced dword loads; the
// decimators to 8 kHz, the split tree, the log energies, the GMM with its model update and FindMinimum
// then run per lane on LDS rows.  Integer arithmetic throughout: bit-exact with the reference.
#include "vad_layout.h"

namespace aspvad {
namespace {

// ------------------------------------------------------------------ register-resident state of one stream
struct Regs {
  int vad;
  int dfs[4];
  int r48[8], r24[16], r16h[8], r8[8];  // WebRtcSpl_State48khzTo8khz: S_48_24, S_24_24, S_24_16, S_16_8
  int16_t* gm;   // the GMM's noise / speech means and stds in LDS, [48][lane]: nm, sm, ns, ss
  int frame_counter, over_hang, num_of_speech;
  int mean_value[6];
  int up[5], lo[5], hp[4];
  int oh1[3], oh2[3], ind[3], tot[3];
  int init_flag;
};

constexpr int kNoiseW[12] = {34, 62, 72, 66, 53, 25, 94, 66, 56, 62, 75, 103};
constexpr int kSpeechW[12] = {48, 82, 45, 87, 50, 47, 80, 46, 83, 41, 78, 81};
constexpr int kSpectrumW[6] = {6, 8, 10, 12, 14, 16};
constexpr int kMinDiff[6] = {544, 544, 576, 576, 576, 576};
constexpr int kMaxSpeech[6] = {11392, 11392, 11520, 11520, 11520, 11520};
constexpr int kMaxNoise[6] = {9216, 9088, 8960, 8832, 8704, 8576};
constexpr int kMinMean[2] = {640, 768};
constexpr int kOffset[6] = {368, 368, 272, 176, 176, 176};

__device__ __forceinline__ void load_state(const AspVadState& g, Regs& r, int16_t* iv, int16_t* lv, int lane) {
  r.vad = g.vad;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.dfs[i] = g.downsampling_filter_states[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r.r48[i] = g.S_48_24[i];
    r.r16h[i] = g.S_24_16[i];
    r.r8[i] = g.S_16_8[i];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) r.r24[i] = g.S_24_24[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    r.gm[(i) * kLanes] = g.noise_means[i];
    r.gm[(12 + i) * kLanes] = g.speech_means[i];
    r.gm[(24 + i) * kLanes] = g.noise_stds[i];
    r.gm[(36 + i) * kLanes] = g.speech_stds[i];
  }
  r.frame_counter = g.frame_counter;
  r.over_hang = g.over_hang;
  r.num_of_speech = g.num_of_speech;
  #pragma unroll 1
  for (int k = 0; k < 96; ++k) {
    iv[k * kLanes + lane] = g.index_vector[k];
    lv[k * kLanes + lane] = g.low_value_vector[k];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) r.mean_value[i] = g.mean_value[i];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    r.up[i] = g.upper_state[i];
    r.lo[i] = g.lower_state[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) r.hp[i] = g.hp_filter_state[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.oh1[i] = g.over_hang_max_1[i];
    r.oh2[i] = g.over_hang_max_2[i];
    r.ind[i] = g.individual[i];
    r.tot[i] = g.total[i];
  }
  r.init_flag = g.init_flag;
}

__device__ __forceinline__ void store_state(AspVadState& g, const Regs& r, const int16_t* iv, const int16_t* lv,
                                            int lane) {
  g.vad = r.vad;
#pragma unroll
  for (int i = 0; i < 4; ++i) g.downsampling_filter_states[i] = r.dfs[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    g.S_48_24[i] = r.r48[i];
    g.S_24_16[i] = r.r16h[i];
    g.S_16_8[i] = r.r8[i];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) g.S_24_24[i] = r.r24[i];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    g.noise_means[i] = (int16_t)r.gm[(i) * kLanes];
    g.speech_means[i] = (int16_t)r.gm[(12 + i) * kLanes];
    g.noise_stds[i] = (int16_t)r.gm[(24 + i) * kLanes];
    g.speech_stds[i] = (int16_t)r.gm[(36 + i) * kLanes];
  }
  g.frame_counter = r.frame_counter;
  g.over_hang = (int16_t)r.over_hang;
  g.num_of_speech = (int16_t)r.num_of_speech;
  #pragma unroll 1
  for (int k = 0; k < 96; ++k) {
    g.index_vector[k] = iv[k * kLanes + lane];
    g.low_value_vector[k] = lv[k * kLanes + lane];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) g.mean_value[i] = (int16_t)r.mean_value[i];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    g.upper_state[i] = (int16_t)r.up[i];
    g.lower_state[i] = (int16_t)r.lo[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) g.hp_filter_state[i] = (int16_t)r.hp[i];
}

// ------------------------------------------------------------------ decimators to 8 kHz
// WebRtcVad_Downsampling's two first-order all-pass branches (vad_sp.c:27-59) on one input pair.
__device__ __forceinline__ int down2(int a, int b, int& t1, int& t2) {
  const int o1 = s16((t1 >> 1) + ((5243 * a) >> 14));
  t1 = a - ((5243 * o1) >> 12);
  const int o2 = s16((t2 >> 1) + ((1392 * b) >> 14));
  t2 = b - ((1392 * o2) >> 12);
  return s16(o1 + o2);
}

// One three-section all-pass of resample_by_2_internal.c on state s[0..3]; returns the new s[3].
template <int C0, int C1, int C2>
__device__ __forceinline__ int ap3(int x, int* s) {
  int d = (wsub(x, s[1]) + (1 << 13)) >> 14;
  const int t1 = wadd(s[0], wmul(d, C0));
  s[0] = x;
  d = wsub(t1, s[2]) >> 14;
  if (d < 0) d += 1;
  const int t0 = wadd(s[1], wmul(d, C1));
  s[1] = t1;
  d = wsub(t0, s[3]) >> 14;
  if (d < 0) d += 1;
  s[3] = wadd(s[2], wmul(d, C2));
  s[2] = t0;
  return s[3];
}
#define AP_LO(x, s) ap3<3050, 9368, 15063>((x), (s))
#define AP_UP(x, s) ap3<821, 6110, 12382>((x), (s))

// WebRtcSpl_Resample48khzTo8khz (resample_48khz.c:103-117) streamed: 12 input samples -> 2 outputs per step,
// the four stages chained through registers (the 8-sample history of the 2/3 stage included).
__device__ __forceinline__ void resample48_to_8(const int16_t* row, int16_t* out8, Regs& r) {
  const int* row32 = reinterpret_cast<const int*>(row);
  #pragma unroll 1
  for (int blk = 0; blk < 40; ++blk) {
    int lp[6];
#pragma unroll
    for (int q = 0; q < 3; ++q) {   // three LPBy2IntToInt pairs <- six DownBy2ShortToInt outputs
      int d[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int w = row32[blk * 6 + q * 2 + h];
        const int xe = (int)(int16_t)(w & 0xFFFF), xo = w >> 16;
        const int lo = AP_LO(wadd(wshl(xe, 15), 1 << 14), &r.r48[0]) >> 1;
        const int up = AP_UP(wadd(wshl(xo, 15), 1 << 14), &r.r48[4]) >> 1;
        d[h] = wadd(lo, up);
      }
      const int ea = AP_LO(r.r24[12], &r.r24[0]) >> 1;   // previous odd input (state[12])
      const int eb = AP_UP(d[0], &r.r24[4]) >> 1;
      const int oa = AP_LO(d[0], &r.r24[8]) >> 1;
      const int ob = AP_UP(d[1], &r.r24[12]) >> 1;
      lp[2 * q] = wadd(ea, eb) >> 15;
      lp[2 * q + 1] = wadd(oa, ob) >> 15;
    }
    int o32[4];
#pragma unroll
    for (int m = 0; m < 2; ++m) {   // Resample48khzTo32khz: 3 in -> 2 out over the 8-sample history
      const int* h = r.r16h;
      const int n0 = lp[3 * m];
      o32[2 * m] = wadd(1 << 14, wadd(wadd(wadd(wmul(778, h[0]), wmul(-2050, h[1])), wadd(wmul(1087, h[2]), wmul(23285, h[3]))),
                                      wadd(wadd(wmul(12903, h[4]), wmul(-3783, h[5])), wadd(wmul(441, h[6]), wmul(222, h[7])))));
      o32[2 * m + 1] = wadd(1 << 14, wadd(wadd(wadd(wmul(222, h[1]), wmul(441, h[2])), wadd(wmul(-3783, h[3]), wmul(12903, h[4]))),
                                          wadd(wadd(wmul(23285, h[5]), wmul(1087, h[6])), wadd(wmul(-2050, h[7]), wmul(778, n0)))));
#pragma unroll
      for (int j = 0; j < 5; ++j) r.r16h[j] = r.r16h[j + 3];
      r.r16h[5] = lp[3 * m];
      r.r16h[6] = lp[3 * m + 1];
      r.r16h[7] = lp[3 * m + 2];
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {   // DownBy2IntToShort with saturation
      const int a = AP_LO(o32[2 * m], &r.r8[0]) >> 1;
      const int b = AP_UP(o32[2 * m + 1], &r.r8[4]) >> 1;
      int v = wadd(a, b) >> 15;
      v = v > 32767 ? 32767 : (v < -32768 ? -32768 : v);
      out8[(blk * 2 + m) * kLanes] = (int16_t)v;
    }
  }
}

// ------------------------------------------------------------------ vad_filterbank.c
// SplitFilter: both all-pass branches in one pass; LDS rows are [n][lane] (stride kLanes).
__device__ __forceinline__ void split(const int16_t* in, int len, int& ust, int& lst, int16_t* hp_out,
                                      int16_t* lp_out) {
  int su = wshl(ust, 16), sl = wshl(lst, 16);
  const int half = len >> 1;
  #pragma unroll 1
  for (int i = 0; i < half; ++i) {
    const int xu = in[(2 * i) * kLanes], xl = in[(2 * i + 1) * kLanes];
    const int tu = s16(wadd(su, 20972 * xu) >> 16);
    su = wshl(wsub(wshl(xu, 14), 20972 * tu), 1);
    const int tl = s16(wadd(sl, 5571 * xl) >> 16);
    sl = wshl(wsub(wshl(xl, 14), 5571 * tl), 1);
    hp_out[i * kLanes] = (int16_t)(tu - tl);
    lp_out[i * kLanes] = (int16_t)(tl + tu);
  }
  ust = s16(su >> 16);
  lst = s16(sl >> 16);
}

__device__ __forceinline__ void high_pass(const int16_t* in, int len, int* st, int16_t* out) {
  #pragma unroll 1
  for (int i = 0; i < len; ++i) {
    const int x = in[i * kLanes];
    int t = 6631 * x - 13262 * st[0] + 6631 * st[1];
    st[1] = st[0];
    st[0] = x;
    t = wadd(t, 7756 * st[2] - 5620 * st[3]);
    st[3] = st[2];
    st[2] = s16(t >> 14);
    out[i * kLanes] = (int16_t)st[2];
  }
}

// LogOfEnergy (vad_filterbank.c:134-245) with WebRtcSpl_Energy / GetScalingSquare.
__device__ __forceinline__ int log_of_energy(const int16_t* in, int len, int offset, int& total) {
  int smax = -1;
  #pragma unroll 1
  for (int i = 0; i < len; ++i) {
    const int x = in[i * kLanes];
    const int a = x > 0 ? x : s16(-x);
    smax = a > smax ? a : smax;
  }
  const int nbits = size_in_bits((unsigned)len);
  const int t = norm_w32(wmul(smax, smax));
  const int scaling = smax == 0 ? 0 : (t > nbits ? 0 : nbits - t);
  int en = 0;
  #pragma unroll 1
  for (int i = 0; i < len; ++i) {
    const int x = in[i * kLanes];
    en = wadd(en, (x * x) >> scaling);
  }
  unsigned e = (unsigned)en;
  if (e == 0) return offset;
  const int nr = 17 - norm_u32(e);
  const int tot = scaling + nr;
  e = nr < 0 ? e << -nr : e >> nr;
  const int log2e = 14336 + (int)((e & 0x3FFF) >> 4);
  int le = s16(((24660 * log2e) >> 19) + ((s16(tot) * 24660) >> 9));
  if (le < 0) le = 0;
  le = s16(le + offset);
  if (total <= 10) total = s16(total + (tot >= 0 ? 11 : s16((int)(e >> -tot))));
  return le;
}

// WebRtcVad_CalculateFeatures: x8 [len][lane] -> f[6], returns the total energy.  b120 / b60 hold the
// split tree's intermediate rows (hp, lp pairs).
__device__ __forceinline__ int features(const int16_t* x8, int len, Regs& r, int16_t* hp120, int16_t* lp120,
                                        int16_t* hp60, int16_t* lp60, int* f) {
  int total = 0;
  const int half = len >> 1, quarter = len >> 2, eighth = len >> 3, sixteenth = len >> 4;
  split(x8, len, r.up[0], r.lo[0], hp120, lp120);
  split(hp120, half, r.up[1], r.lo[1], hp60, lp60);
  f[5] = log_of_energy(hp60, quarter, kOffset[5], total);
  f[4] = log_of_energy(lp60, quarter, kOffset[4], total);
  split(lp120, half, r.up[2], r.lo[2], hp60, lp60);
  f[3] = log_of_energy(hp60, quarter, kOffset[3], total);
  split(lp60, quarter, r.up[3], r.lo[3], hp120, lp120);
  f[2] = log_of_energy(hp120, eighth, kOffset[2], total);
  split(lp120, eighth, r.up[4], r.lo[4], hp60, lp60);
  f[1] = log_of_energy(hp60, sixteenth, kOffset[1], total);
  high_pass(lp60, sixteenth, r.hp, hp120);
  f[0] = log_of_energy(hp120, sixteenth, kOffset[0], total);
  return total;
}

// ------------------------------------------------------------------ vad_gmm.c
__device__ __forceinline__ int gaussian(int input, int mean, int std_, int& delta) {
  const int inv_std = s16(div_w32w16(131072 + (std_ >> 1), std_));
  int t16 = inv_std >> 2;
  const int inv_std2 = s16((t16 * t16) >> 2);
  t16 = s16(s16(wshl(input, 3)) - mean);
  delta = s16((inv_std2 * t16) >> 10);
  const int e32 = (delta * t16) >> 9;
  int ev = 0;
  if (e32 < 22005) {
    int t = s16((5909 * s16(e32)) >> 12);
    t = s16(-t);
    ev = 0x0400 | (t & 0x03FF);
    t = s16(~t);
    t = (t >> 10) + 1;
    ev = ev >> (t & 31);
  }
  return inv_std * ev;
}

// ------------------------------------------------------------------ vad_sp.c FindMinimum on the LDS vectors
__device__ __forceinline__ int find_minimum(Regs& r, int16_t* iv, int16_t* lv, int feature, int ch, int lane) {
  int16_t* age = iv + ch * 16 * kLanes + lane;
  int16_t* sv = lv + ch * 16 * kLanes + lane;
  #pragma unroll 1
  for (int i = 0; i < 16; ++i) {
    if (age[i * kLanes] != 100) {
      age[i * kLanes] = (int16_t)(age[i * kLanes] + 1);
    } else {   // the oldest value leaves; the larger ones move down
      #pragma unroll 1
      for (int j = i; j < 15; ++j) {
        sv[j * kLanes] = sv[(j + 1) * kLanes];
        age[j * kLanes] = age[(j + 1) * kLanes];
      }
      age[15 * kLanes] = 101;
      sv[15 * kLanes] = 10000;
    }
  }
  // the reference's binary search over the sorted values, restated as the same decision tree
  auto lt = [&](int k) { return feature < sv[k * kLanes]; };
  int pos = -1;
  if (lt(7)) {
    if (lt(3)) pos = lt(1) ? (lt(0) ? 0 : 1) : (lt(2) ? 2 : 3);
    else pos = lt(5) ? (lt(4) ? 4 : 5) : (lt(6) ? 6 : 7);
  } else if (lt(15)) {
    if (lt(11)) pos = lt(9) ? (lt(8) ? 8 : 9) : (lt(10) ? 10 : 11);
    else pos = lt(13) ? (lt(12) ? 12 : 13) : (lt(14) ? 14 : 15);
  }
  if (pos >= 0) {
    #pragma unroll 1
    for (int i = 15; i > pos; --i) {
      sv[i * kLanes] = sv[(i - 1) * kLanes];
      age[i * kLanes] = age[(i - 1) * kLanes];
    }
    sv[pos * kLanes] = (int16_t)feature;
    age[pos * kLanes] = 1;
  }
  int med = 1600;
  if (r.frame_counter > 2) med = sv[2 * kLanes];
  else if (r.frame_counter > 0) med = sv[0];
  int alpha = 0;
  if (r.frame_counter > 0) alpha = med < r.mean_value[ch] ? 6553 : 32439;
  const int t = (alpha + 1) * r.mean_value[ch] + (32767 - alpha) * med + 16384;
  r.mean_value[ch] = s16(t >> 15);
  return r.mean_value[ch];
}

// ------------------------------------------------------------------ vad_core.c GmmProbability
__device__ __forceinline__ int gmm(Regs& r, const int* f, int total_power, int len8, int16_t* iv, int16_t* lv,
                                   int lane) {
  const int li = len8 == 80 ? 0 : (len8 == 160 ? 1 : 2);
  // selects, not a runtime index: the tables stay in registers
  auto pick = [li](const int* t) { return li == 0 ? t[0] : (li == 1 ? t[1] : t[2]); };
  const int oh1 = pick(r.oh1), oh2 = pick(r.oh2), ind = pick(r.ind), totT = pick(r.tot);
  int vadflag = 0;
  if (total_power > 10) {
    int dN[12], dS[12], ng[12], sg[12];
    int sum_llr = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      int h0 = 0, h1 = 0, np0 = 0, sp0 = 0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int g = c + 6 * k;
        const int pn = wmul(kNoiseW[g], gaussian(f[c], r.gm[(g) * kLanes], r.gm[(24 + g) * kLanes], dN[g]));
        const int ps = wmul(kSpeechW[g], gaussian(f[c], r.gm[(12 + g) * kLanes], r.gm[(36 + g) * kLanes], dS[g]));
        if (k == 0) {
          np0 = pn;
          sp0 = ps;
        }
        h0 = wadd(h0, pn);
        h1 = wadd(h1, ps);
      }
      const int sh0 = h0 == 0 ? 31 : norm_w32(h0);
      const int sh1 = h1 == 0 ? 31 : norm_w32(h1);
      const int llr = s16(sh0 - sh1);
      sum_llr = wadd(sum_llr, llr * kSpectrumW[c]);
      if (wshl(llr, 2) > ind) vadflag = 1;
      const int h0s = s16(h0 >> 12);
      if (h0s > 0) {
        ng[c] = s16(div_w32w16((int)(((unsigned)np0 & 0xFFFFF000u) << 2), h0s));
        ng[c + 6] = s16(16384 - ng[c]);
      } else {
        ng[c] = 16384;
        ng[c + 6] = 0;
      }
      const int h1s = s16(h1 >> 12);
      if (h1s > 0) {
        sg[c] = s16(div_w32w16((int)(((unsigned)sp0 & 0xFFFFF000u) << 2), h1s));
        sg[c + 6] = s16(16384 - sg[c]);
      } else {
        sg[c] = 0;
        sg[c + 6] = 0;
      }
    }
    vadflag |= (sum_llr >= totT);

    int maxspe = 12800;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const int fmin = find_minimum(r, iv, lv, f[c], c, lane);
      int ngm = kNoiseW[c] * r.gm[(c) * kLanes] + kNoiseW[c + 6] * r.gm[(c + 6) * kLanes];
      const int t1g = s16(ngm >> 6);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int g = c + 6 * k;
        const int nmk = r.gm[(g) * kLanes], smk = r.gm[(12 + g) * kLanes], nsk = r.gm[(24 + g) * kLanes], ssk = r.gm[(36 + g) * kLanes];
        int nmk2 = nmk;
        if (!vadflag) {
          const int delt = s16((ng[g] * dN[g]) >> 11);
          nmk2 = s16(nmk + s16((delt * 655) >> 22));
        }
        const int ndelt = s16(wshl(fmin, 4) - t1g);
        int nmk3 = s16(nmk2 + s16((ndelt * 154) >> 9));
        if (nmk3 < ((k + 5) << 7)) nmk3 = (k + 5) << 7;
        if (nmk3 > ((72 + k - c) << 7)) nmk3 = (72 + k - c) << 7;
        r.gm[(g) * kLanes] = nmk3;
        if (vadflag) {
          const int delt = s16((sg[g] * dS[g]) >> 11);
          const int t = s16((delt * 6554) >> 21);
          int smk2 = s16(smk + ((t + 1) >> 1));
          const int maxmu = s16(maxspe + 640);
          if (smk2 < kMinMean[k]) smk2 = kMinMean[k];
          if (smk2 > maxmu) smk2 = maxmu;
          r.gm[(12 + g) * kLanes] = smk2;
          const int d16 = s16(f[c] - ((smk + 4) >> 3));
          const int a32 = wsub((dS[g] * d16) >> 3, 4096);
          const int b32 = wmul(sg[g] >> 2, a32) >> 4;
          int q;
          if (b32 > 0) q = s16(div_w32w16(b32, ssk * 10));
          else q = s16(-s16(div_w32w16(wsub(0, b32), ssk * 10)));
          q = s16(q + 128);
          int ssk2 = s16(ssk + (q >> 8));
          if (ssk2 < 384) ssk2 = 384;
          r.gm[(36 + g) * kLanes] = ssk2;
        } else {
          const int d16 = s16(f[c] - (nmk >> 3));
          const int a32 = wsub((dN[g] * d16) >> 3, 4096);
          const int b32 = wmul((ng[g] + 2) >> 2, a32) >> 14;
          int q;
          if (b32 > 0) q = s16(div_w32w16(b32, nsk));
          else q = s16(-s16(div_w32w16(wsub(0, b32), nsk)));
          q = s16(q + 32);
          int nsk2 = s16(nsk + (q >> 6));
          if (nsk2 < 384) nsk2 = 384;
          r.gm[(24 + g) * kLanes] = nsk2;
        }
      }
      ngm = wadd(wmul(kNoiseW[c], r.gm[(c) * kLanes]), wmul(kNoiseW[c + 6], r.gm[(c + 6) * kLanes]));
      int sgm = wadd(wmul(kSpeechW[c], r.gm[(12 + c) * kLanes]), wmul(kSpeechW[c + 6], r.gm[(12 + c + 6) * kLanes]));
      const int diff = s16(s16(sgm >> 9) - s16(ngm >> 9));
      if (diff < kMinDiff[c]) {
        const int t = s16(kMinDiff[c] - diff);
        const int t1 = s16((13 * t) >> 2), t2 = s16((3 * t) >> 2);
        r.gm[(12 + c) * kLanes] = s16(r.gm[(12 + c) * kLanes] + t1);
        r.gm[(12 + c + 6) * kLanes] = s16(r.gm[(12 + c + 6) * kLanes] + t1);
        sgm = wadd(wmul(kSpeechW[c], r.gm[(12 + c) * kLanes]), wmul(kSpeechW[c + 6], r.gm[(12 + c + 6) * kLanes]));
        r.gm[(c) * kLanes] = s16(r.gm[(c) * kLanes] - t2);
        r.gm[(c + 6) * kLanes] = s16(r.gm[(c + 6) * kLanes] - t2);
        ngm = wadd(wmul(kNoiseW[c], r.gm[(c) * kLanes]), wmul(kNoiseW[c + 6], r.gm[(c + 6) * kLanes]));
      }
      maxspe = kMaxSpeech[c];
      int t = s16(sgm >> 7);
      if (t > maxspe) {
        r.gm[(12 + c) * kLanes] = s16(r.gm[(12 + c) * kLanes] - (t - maxspe));
        r.gm[(12 + c + 6) * kLanes] = s16(r.gm[(12 + c + 6) * kLanes] - (t - maxspe));
      }
      t = s16(ngm >> 7);
      if (t > kMaxNoise[c]) {
        r.gm[(c) * kLanes] = s16(r.gm[(c) * kLanes] - (t - kMaxNoise[c]));
        r.gm[(c + 6) * kLanes] = s16(r.gm[(c + 6) * kLanes] - (t - kMaxNoise[c]));
      }
    }
    r.frame_counter = wadd(r.frame_counter, 1);
  }
  // hangover
  if (!vadflag) {
    if (r.over_hang > 0) {
      vadflag = s16(2 + r.over_hang);
      r.over_hang = s16(r.over_hang - 1);
    }
    r.num_of_speech = 0;
  } else {
    r.num_of_speech = s16(r.num_of_speech + 1);
    if (r.num_of_speech > 6) {
      r.num_of_speech = 6;
      r.over_hang = oh2;
    } else {
      r.over_hang = oh1;
    }
  }
  return vadflag;
}

// ------------------------------------------------------------------ the kernel
struct Lds {
  union {
    int16_t in[kLanes * kInStride];   // staged 10 ms piece, [lane][kInStride]
    struct {
      int16_t hp120[120 * kLanes], lp120[120 * kLanes], hp60[60 * kLanes], lp60[60 * kLanes];
    } fb;
  } u;
  int16_t x8[kMax8k * kLanes];       // the frame at 8 kHz, [n][lane]
  int16_t iv[96 * kLanes], lv[96 * kLanes];
  int16_t gm[48 * kLanes];
};

// Stage samples [off, off + P) of every stream's frame into LDS (coalesced: consecutive lanes read
// consecutive dwords of one stream's row).
__device__ __forceinline__ void stage(Lds& lds, const int16_t* in, size_t frame_base, int S, int s0, int L, int off,
                                      int P, int lane) {
  const int words = P >> 1;
  int* dst = reinterpret_cast<int*>(lds.u.in);
  #pragma unroll 1
  for (int j = lane; j < kLanes * words; j += kLanes) {
    const int row = j / words, c = j - row * words;
    const int s = s0 + row;
    if (s < S) {
      const int* src = reinterpret_cast<const int*>(in + frame_base + (size_t)s * L + off);
      dst[row * (kInStride / 2) + c] = src[c];
    }
  }
}

__global__ __launch_bounds__(kLanes) void vad_process_kernel(AspVadState* __restrict__ state,
                                                             const int16_t* __restrict__ in, int S, int fs, int L,
                                                             int F, int8_t* __restrict__ dec,
                                                             int32_t* __restrict__ lev, int16_t* __restrict__ feat) {
  __shared__ Lds lds;
  const int lane = threadIdx.x;
  const int s0 = blockIdx.x * kLanes;
  const int s = s0 + lane;
  const bool valid = s < S;
  Regs r;
  r.gm = lds.gm + lane;
  load_state(state[valid ? s : S - 1], r, lds.iv, lds.lv, lane);
  const int P = fs / 100;                 // samples per 10 ms
  const int n10 = L / P;                  // 10 ms pieces per frame
  const int len8 = 80 * n10;
  const int16_t* row = lds.u.in + lane * kInStride;
  for (int f = 0; f < F; ++f) {
    const size_t frame_base = (size_t)f * S * L;
    if (fs == 48000) {
      // CalcVad48khz resamples the frame's first 10 ms once per 10 ms of the frame (vad_core.c:618-623)
      stage(lds, in, frame_base, S, s0, L, 0, 480, lane);
      __syncthreads();
      #pragma unroll 1
      for (int i = 0; i < n10; ++i) resample48_to_8(row, lds.x8 + i * 80 * kLanes + lane, r);
    } else {
      #pragma unroll 1
      for (int p = 0; p < n10; ++p) {
        stage(lds, in, frame_base, S, s0, L, p * P, P, lane);
        __syncthreads();
        int16_t* o = lds.x8 + p * 80 * kLanes + lane;
        const int* row32 = reinterpret_cast<const int*>(row);
        if (fs == 8000) {
          #pragma unroll 1
          for (int n = 0; n < 80; ++n) o[n * kLanes] = row[n];
        } else if (fs == 16000) {
          #pragma unroll 1
          for (int n = 0; n < 80; ++n) {
            const int w = row32[n];
            o[n * kLanes] = (int16_t)down2((int)(int16_t)(w & 0xFFFF), w >> 16, r.dfs[0], r.dfs[1]);
          }
        } else {   // 32 -> 16 -> 8 kHz
          #pragma unroll 1
          for (int n = 0; n < 80; ++n) {
            const int w0 = row32[2 * n], w1 = row32[2 * n + 1];
            const int a = down2((int)(int16_t)(w0 & 0xFFFF), w0 >> 16, r.dfs[2], r.dfs[3]);
            const int b = down2((int)(int16_t)(w1 & 0xFFFF), w1 >> 16, r.dfs[2], r.dfs[3]);
            o[n * kLanes] = (int16_t)down2(a, b, r.dfs[0], r.dfs[1]);
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();   // the split tree's rows alias the staging buffer
    int fv[6];
    const int total = features(lds.x8 + lane, len8, r, lds.u.fb.hp120 + lane, lds.u.fb.lp120 + lane,
                               lds.u.fb.hp60 + lane, lds.u.fb.lp60 + lane, fv);
    if (feat) {   // the CalculateFeatures seam: no GMM
      if (valid) {
#pragma unroll
        for (int c = 0; c < 6; ++c) feat[(size_t)s * 7 + c] = (int16_t)fv[c];
        feat[(size_t)s * 7 + 6] = (int16_t)total;
      }
    } else {
      const int v = gmm(r, fv, total, len8, lds.iv, lds.lv, lane);
      r.vad = v;
      if (valid) {
        dec[(size_t)f * S + s] = v > 0 ? 1 : 0;
        if (lev) lev[(size_t)f * S + s] = v;
      }
    }
    __syncthreads();   // the next frame's staging overwrites the split tree's rows
  }
  if (valid) store_state(state[s], r, lds.iv, lds.lv, lane);
}

// InitCore (init != 0) and / or set_mode_core for streams [first, first + count)
__global__ void vad_init_kernel(AspVadState* __restrict__ state, int first, int count, int init, int mode) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  AspVadState& g = state[first + i];
  if (init) {
    constexpr int16_t kNM[12] = {6738, 4892, 7065, 6715, 6771, 3369, 7646, 3863, 7820, 7266, 5020, 4362};
    constexpr int16_t kSM[12] = {8306, 10085, 10078, 11823, 11843, 6309, 9473, 9571, 10879, 7581, 8180, 7483};
    constexpr int16_t kNS[12] = {378, 1064, 493, 582, 688, 593, 474, 697, 475, 688, 421, 455};
    constexpr int16_t kSS[12] = {555, 505, 567, 524, 585, 1231, 509, 828, 492, 1540, 1079, 850};
    g.vad = 1;
    g.frame_counter = 0;
    g.over_hang = 0;
    g.num_of_speech = 0;
    for (int k = 0; k < 4; ++k) g.downsampling_filter_states[k] = 0;
    for (int k = 0; k < 8; ++k) g.S_48_24[k] = g.S_24_16[k] = g.S_16_8[k] = 0;
    for (int k = 0; k < 16; ++k) g.S_24_24[k] = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      g.noise_means[k] = kNM[k];
      g.speech_means[k] = kSM[k];
      g.noise_stds[k] = kNS[k];
      g.speech_stds[k] = kSS[k];
    }
    #pragma unroll 1
  for (int k = 0; k < 96; ++k) {
      g.low_value_vector[k] = 10000;
      g.index_vector[k] = 0;
    }
    for (int k = 0; k < 5; ++k) g.upper_state[k] = g.lower_state[k] = 0;
    for (int k = 0; k < 4; ++k) g.hp_filter_state[k] = 0;
    for (int k = 0; k < 6; ++k) g.mean_value[k] = 1600;
    g.init_flag = kInitCheck;
  }
  mode_table(mode, g.over_hang_max_1, g.over_hang_max_2, g.individual, g.total);
}

__global__ void vad_gaussian_kernel(const int16_t* in, const int16_t* mean, const int16_t* std_, int n, int32_t* p,
                                    int16_t* delta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int d = 0;
  p[i] = gaussian(in[i], mean[i], std_[i], d);
  delta[i] = (int16_t)d;
}

}  // namespace

hipError_t launch_process(AspVadState* state, const int16_t* in, int S, int fs, int L, int F, int8_t* dec,
                          int32_t* lev, int16_t* feat, hipStream_t st) {
  hipLaunchKernelGGL(vad_process_kernel, dim3((S + kLanes - 1) / kLanes), dim3(kLanes), 0, st, state, in, S, fs, L,
                     F, dec, lev, feat);
  return hipGetLastError();
}

hipError_t launch_init(AspVadState* state, int first, int count, int init, int mode, hipStream_t st) {
  hipLaunchKernelGGL(vad_init_kernel, dim3((count + 255) / 256), dim3(256), 0, st, state, first, count, init, mode);
  return hipGetLastError();
}

hipError_t launch_gaussian(const int16_t* in, const int16_t* mean, const int16_t* std_, int n, int32_t* p,
                           int16_t* delta, hipStream_t st) {
  hipLaunchKernelGGL(vad_gaussian_kernel, dim3((n + 255) / 256), dim3(256), 0, st, in, mean, std_, n, p, delta);
  return hipGetLastError();
}

}  // namespace aspvad
