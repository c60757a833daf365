// bf_ref_shim.cc -- extern "C" access to the reference's webrtc::Beamformer for tests/golden/make_bf_golden.py
// (the compile line is in that script's docstring).  Two parts:
//
// 1. The FFT seam.  webrtc::RealFourier calls four omxSP_* functions of OpenMAX DL, which the reference snapshot
//    does not contain.  They are defined here on the reference's own WebRtc_rdft (fft4g.c, compiled in place):
//    forward is rdft(n, +1, a) repacked as CCS (bin 0 = (a[0], 0), bin k = (a[2k], -a[2k+1]), bin n/2 =
//    (a[1], 0)); inverse is the same packing back, rdft(n, -1, a), every sample times 2.0f / n.
// 2. create / Initialize / ProcessChunk / is_target_present and copies of private members (opened below).  The
//    subclass only records the mask row of every block; with `probe` set it also forgets the previous block
//    before each one, so that ApplyDecay is skipped and the row holds the masks as CalculatePostfilterMask left
//    them (bins below the mid band are the low-frequency mean).  No algorithm here.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <complex>
#include <sstream>
#include <string>
#include <vector>

#include "third_party/openmax_dl/dl/sp/api/omxSP.h"

#define private public
#define protected public
#include "webrtc/common_audio/blocker.h"
#include "webrtc/common_audio/lapped_transform.h"
#include "webrtc/common_audio/real_fourier.h"
#include "webrtc/modules/audio_processing/beamformer/beamformer.h"
#undef private
#undef protected

extern "C" void WebRtc_rdft(int n, int isgn, float* a, int* ip, float* w);

// ------------------------------------------------------------------------------------------- the FFT seam
namespace {
struct Spec {
  int n;
  int ip[2 + 64];     // 2 + sqrt(n / 2) for n <= 4096
  float w[2048];      // n / 2
  float a[4096];      // n
};
}  // namespace

extern "C" {
OMXResult omxSP_FFTGetBufSize_R_F32(OMX_INT order, OMX_INT* size) {
  if (order < 1 || order > TWIDDLE_TABLE_ORDER || !size) return OMX_Sts_BadArgErr;
  *size = (OMX_INT)sizeof(Spec);
  return OMX_Sts_NoErr;
}
OMXResult omxSP_FFTInit_R_F32(OMXFFTSpec_R_F32* spec, OMX_INT order) {
  if (!spec || order < 1 || order > TWIDDLE_TABLE_ORDER) return OMX_Sts_BadArgErr;
  Spec* s = (Spec*)spec;
  memset(s, 0, sizeof *s);
  s->n = 1 << order;  // ip[0] == 0: the first transform makes the tables
  return OMX_Sts_NoErr;
}
OMXResult omxSP_FFTFwd_RToCCS_F32(const OMX_F32* src, OMX_F32* dst, const OMXFFTSpec_R_F32* spec) {
  Spec* s = (Spec*)spec;
  const int n = s->n;
  memcpy(s->a, src, sizeof(float) * n);
  WebRtc_rdft(n, 1, s->a, s->ip, s->w);
  dst[0] = s->a[0];
  dst[1] = 0.f;
  for (int k = 1; k < n / 2; ++k) {
    dst[2 * k] = s->a[2 * k];
    dst[2 * k + 1] = -s->a[2 * k + 1];
  }
  dst[n] = s->a[1];
  dst[n + 1] = 0.f;
  return OMX_Sts_NoErr;
}
OMXResult omxSP_FFTInv_CCSToR_F32(const OMX_F32* src, OMX_F32* dst, const OMXFFTSpec_R_F32* spec) {
  Spec* s = (Spec*)spec;
  const int n = s->n;
  s->a[0] = src[0];
  s->a[1] = src[n];
  for (int k = 1; k < n / 2; ++k) {
    s->a[2 * k] = src[2 * k];
    s->a[2 * k + 1] = -src[2 * k + 1];
  }
  WebRtc_rdft(n, -1, s->a, s->ip, s->w);
  const float scale = 2.0f / n;
  for (int j = 0; j < n; ++j) dst[j] = s->a[j] * scale;
  return OMX_Sts_NoErr;
}
}  // extern "C"

// ------------------------------------------------------------------------------------------- the beamformer
namespace {
const int kBins = 129;

struct Rec : webrtc::Beamformer {
  Rec(const std::vector<webrtc::Point>& g, bool probe) : webrtc::Beamformer(g), probe(probe) {}
  void ProcessAudioBlock(const std::complex<float>* const* input, int num_input_channels, int num_freq_bins,
                         int num_output_channels, std::complex<float>* const* output) override {
    if (probe) previous_block_ix_ = -1;
    webrtc::Beamformer::ProcessAudioBlock(input, num_input_channels, num_freq_bins, num_output_channels, output);
    const float* row = postfilter_masks_[previous_block_ix_].elements()[0];
    log.insert(log.end(), row, row + kBins);
  }
  bool probe;
  std::vector<float> log;
};

int copy_cplx(const webrtc::ComplexMatrix<float>* mats, float* out) {
  int n = 0;
  for (int f = 0; f < kBins; ++f)
    for (int r = 0; r < mats[f].num_rows(); ++r)
      for (int c = 0; c < mats[f].num_columns(); ++c) {
        out[n++] = mats[f].elements()[r][c].real();
        out[n++] = mats[f].elements()[r][c].imag();
      }
  return n;
}
}  // namespace

extern "C" {
void* bf_ref_create(const float* xyz, int num_mics, int probe) {
  std::vector<webrtc::Point> g;
  for (int i = 0; i < num_mics; ++i) g.push_back(webrtc::Point(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
  Rec* b = new Rec(g, probe != 0);
  // the reference never initialises this member and reads it in the first chunk's high-band ramp; the
  // specification starts it at 0
  b->high_pass_postfilter_mask_ = 0.f;
  return b;
}
void bf_ref_free(void* h) { delete (Rec*)h; }
void bf_ref_initialize(void* h, int chunk_size_ms, int sample_rate_hz) {
  ((Rec*)h)->Initialize(chunk_size_ms, sample_rate_hz);
}
// input [M][L], high [M][L] or NULL, output [L], high_output [L] (untouched without a high band)
void bf_ref_process(void* h, const float* input, const float* high, float* output, float* high_output) {
  Rec* b = (Rec*)h;
  const int M = b->num_input_channels_, L = b->chunk_length_;
  std::vector<const float*> in(M), hi(M);
  for (int c = 0; c < M; ++c) {
    in[c] = input + (size_t)c * L;
    hi[c] = high ? high + (size_t)c * L : nullptr;
  }
  float* out[1] = {output};
  float* hout[1] = {high_output};
  b->ProcessChunk(in.data(), high ? hi.data() : nullptr, M, L, out, hout);
}
int bf_ref_is_target_present(void* h) { return ((Rec*)h)->is_target_present() ? 1 : 0; }

// frame_offset_, current_block_ix_, previous_block_ix_, is_target_present_, interference_blocks_count_,
// hold_target_blocks_, the four bin bounds (mid lower, mid upper, high lower, high upper), initial_delay_,
// chunk_length_
void bf_ref_ints(void* h, int32_t* out) {
  Rec* b = (Rec*)h;
  webrtc::Blocker* k = b->lapped_transform_->blocker_.get();
  out[0] = k->frame_offset_;
  out[1] = b->current_block_ix_;
  out[2] = b->previous_block_ix_;
  out[3] = b->is_target_present_;
  out[4] = b->interference_blocks_count_;
  out[5] = b->hold_target_blocks_;
  out[6] = b->mid_frequency_lower_bin_bound_;
  out[7] = b->mid_frequency_upper_bin_bound_;
  out[8] = b->high_frequency_lower_bin_bound_;
  out[9] = b->high_frequency_upper_bin_bound_;
  out[10] = k->initial_delay_;
  out[11] = b->chunk_length_;
}

// which: 0 window_, 1 wave_numbers_, 2 mask_thresholds_, 3 delay_sum_masks_ [bins][M][2], 4 target_cov_mats_
// [bins][M][M][2], 5 interf_cov_mats_, 6 rxiws_, 7 rpsiws_, 8 reflected_rpsiws_, 9 decay_threshold_,
// 10 reflected_interf_cov_mats_, 11 the blocker's input buffer [M][384], 12 its output buffer [384],
// 13 postfilter_masks_ [2][bins], 14 high_pass_postfilter_mask_, 15 mic_spacing_; returns the count
int bf_ref_array(void* h, int which, float* out) {
  Rec* b = (Rec*)h;
  const int M = b->num_input_channels_;
  const float* p = nullptr;
  int n = kBins;
  switch (which) {
    case 0: p = b->window_; n = 256; break;
    case 1: p = b->wave_numbers_; break;
    case 2: p = b->mask_thresholds_; break;
    case 3: return copy_cplx(b->delay_sum_masks_, out);
    case 4: return copy_cplx(b->target_cov_mats_, out);
    case 5: return copy_cplx(b->interf_cov_mats_, out);
    case 6: p = b->rxiws_; break;
    case 7: p = b->rpsiws_; break;
    case 8: p = b->reflected_rpsiws_; break;
    case 9: p = &b->decay_threshold_; n = 1; break;
    case 10: return copy_cplx(b->reflected_interf_cov_mats_, out);
    case 11:
    case 12: {
      webrtc::Blocker* k = b->lapped_transform_->blocker_.get();
      const int len = k->chunk_size_ + k->initial_delay_, C = which == 11 ? M : 1;
      float* const* ch = which == 11 ? k->input_buffer_.channels() : k->output_buffer_.channels();
      for (int c = 0; c < C; ++c) memcpy(out + (size_t)c * len, ch[c], sizeof(float) * len);
      return C * len;
    }
    case 13:
      for (int r = 0; r < 2; ++r) memcpy(out + r * kBins, b->postfilter_masks_[r].elements()[0], sizeof(float) * kBins);
      return 2 * kBins;
    case 14: p = &b->high_pass_postfilter_mask_; n = 1; break;
    case 15: p = &b->mic_spacing_; n = 1; break;
    default: return -1;
  }
  memcpy(out, p, sizeof(float) * n);
  return n;
}

// the mask rows recorded since the last call, [rows][bins]; returns rows and clears the record
int bf_ref_mask_log(void* h, float* out, int cap_rows) {
  Rec* b = (Rec*)h;
  const int rows = (int)(b->log.size() / kBins);
  if (rows > cap_rows) return -1;
  if (rows) memcpy(out, b->log.data(), sizeof(float) * b->log.size());
  b->log.clear();
  return rows;
}

// webrtc::RealFourier over the seam, for the generator's two checks: x [n] -> ccs [n / 2 + 1][2] and back
void bf_ref_fft(int n, const float* x, float* ccs, float* back) {
  webrtc::RealFourier f(webrtc::RealFourier::FftOrder(n));
  std::vector<std::complex<float> > c(n / 2 + 1);
  f.Forward(x, c.data());
  memcpy(ccs, c.data(), sizeof(float) * (n + 2));
  f.Inverse(c.data(), back);
}
}
