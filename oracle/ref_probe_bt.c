/*
 * ref_probe_bt.c -- glue compiled INTO oracle/_ref/libbt_ref.so around the reference's own
 * Denoise/BlockThresholding/src/audioDenoiseBlockTreshold.c, which is compiled in place by the
 * two #includes below (see oracle/Makefile).  TEST INFRASTRUCTURE ONLY.  It contains no
 * algorithm of the reference.
 *
 * The FFT seam.  audioDenoiseBlockTreshold.c needs three external symbols, kiss_fftr_alloc,
 * kiss_fftr and kiss_fftri; the reference's kiss_fft cannot be built (its _kiss_fft_guts.h is
 * not in the tree), so the three are defined here and forward to the oracle's restatement of
 * kiss_fft (bt_oracle.c, compiled into the same library).  Everything else in the library --
 * window, framing, SURE segmentation, thresholds, Wiener step, overlap-add, flush, the int16
 * conversions, return codes -- is the reference's object code.
 *
 * asp_bt.h / bt_oracle.h are NOT included: they declare the same blockThreshold_* names (with
 * an opaque handle).  The few oracle functions used are declared by hand.
 *
 * The reference's header declares blockThreshold_flush_float(handle, float*, int32_t) while the
 * definition takes int16_t* (.h:66 against .c:648; it memcpy's floats): the header's
 * declaration is renamed around the include so that the definition compiles.  Callers pass a
 * float buffer through void*.
 */
#define blockThreshold_flush_float blockThreshold_flush_float_as_declared_in_the_header
#include "Denoise/BlockThresholding/src/audioDenoiseBlockTreshold.h"
#undef blockThreshold_flush_float
#include "Denoise/BlockThresholding/src/audioDenoiseBlockTreshold.c"

typedef struct BtOracle BtOracle;
BtOracle* bt_oracle_create(int win_size);
void bt_oracle_free(BtOracle* h);
void bt_oracle_kiss_fftr(BtOracle* h, const float* timedata, float* freq);
void bt_oracle_kiss_fftri(BtOracle* h, const float* freq, float* timedata);

/* kiss_fftr_free is free() (kiss_fftr.h:41): the configuration object is one malloc block.  The
 * oracle handle it points to is released by ref_bt_free below, ahead of blockThreshold_free. */
struct kiss_fftr_state {
  BtOracle* fft;
};

kiss_fftr_cfg kiss_fftr_alloc(int nfft, int inverse_fft, void* mem, size_t* lenmem) {
  (void)inverse_fft; /* one oracle handle carries both directions */
  if (mem || lenmem) return NULL;
  BtOracle* o = bt_oracle_create(nfft);
  if (!o) return NULL;
  kiss_fftr_cfg cfg = (kiss_fftr_cfg)malloc(sizeof(struct kiss_fftr_state));
  cfg->fft = o;
  return cfg;
}

void kiss_fftr(kiss_fftr_cfg cfg, const kiss_fft_scalar* timedata, kiss_fft_cpx* freqdata) {
  bt_oracle_kiss_fftr(cfg->fft, timedata, (float*)freqdata);
}

void kiss_fftri(kiss_fftr_cfg cfg, const kiss_fft_cpx* freqdata, kiss_fft_scalar* timedata) {
  bt_oracle_kiss_fftri(cfg->fft, (const float*)freqdata, timedata);
}

void ref_bt_free(MarsBlockThreshold_t* h) {
  if (!h) return;
  bt_oracle_free(h->forward_fftr_cfg->fft);
  bt_oracle_free(h->backward_fftr_cfg->fft);
  blockThreshold_free(h);
}

/* ---- views of the handle */
int32_t ref_bt_win(const MarsBlockThreshold_t* h) { return h->win_size; }
int32_t ref_bt_have(const MarsBlockThreshold_t* h) { return h->have_nblk_time; }
const float* ref_bt_hann(const MarsBlockThreshold_t* h) { return h->win_hanning; }
const float* ref_bt_inbuf(const MarsBlockThreshold_t* h) { return h->inbuf; }   /* [win_size] */
const float* ref_bt_outbuf(const MarsBlockThreshold_t* h) { return h->outbuf; } /* [macro_size + half_win_size] */

/* spectrum of cached hop `row` (0 .. have_nblk_time - 1): [win_size / 2 + 1] interleaved {r, i} */
void ref_bt_coef(const MarsBlockThreshold_t* h, int row, float* out) {
  memcpy(out, h->stft_coef[row], sizeof(kiss_fft_cpx) * (size_t)(h->win_size / 2 + 1));
}

/* ---- the static conversions */
void ref_bt_s16_to_float(const int16_t* v, float* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = S16ToFloat(v[i]);
}
void ref_bt_float_to_s16(const float* v, int16_t* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = FloatToS16(v[i]);
}

/* ---- the static core on caller-supplied spectra: coef [8][win/2 + 1] interleaved {r, i}, replaced by
 * stft_coef after the Wiener step; thre the same shape, stft_thre; per macro-column c a direct call of
 * blockThreshold_adaptive_block on the spectra as given: seg[2 c] = seg_time, seg[2 c + 1] = seg_freq,
 * sure[15 c ..] the 3 x 5 SURE_matrix it left. */
void ref_bt_core(MarsBlockThreshold_t* h, float* coef, float* thre, int32_t* seg, float* sure) {
  const int nb = h->win_size / 2 + 1;
  const int ncol = (h->win_size - 1) / 2 / h->max_nblk_freq;
  for (int t = 0; t < h->max_nblk_time; ++t)
    memcpy(h->stft_coef[t], coef + (size_t)t * 2 * nb, sizeof(kiss_fft_cpx) * (size_t)nb);
  for (int c = 0; c < ncol; ++c) {
    blockThreshold_adaptive_block(h, c, &seg[2 * c], &seg[2 * c + 1]);
    for (int i = 0; i < h->nblk_time; ++i)
      memcpy(sure + 15 * c + 5 * i, h->SURE_matrix[i], sizeof(float) * (size_t)h->nblk_freq);
  }
  blockThreshold_core(h);
  for (int t = 0; t < h->max_nblk_time; ++t) {
    memcpy(coef + (size_t)t * 2 * nb, h->stft_coef[t], sizeof(kiss_fft_cpx) * (size_t)nb);
    memcpy(thre + (size_t)t * 2 * nb, h->stft_thre[t], sizeof(kiss_fft_cpx) * (size_t)nb);
  }
}
