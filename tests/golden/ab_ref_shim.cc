// ab_ref_shim.cc -- access code for tests/golden/make_ab_golden.py, compiled against the reference in the build
// container only (the compile line is in the generator's docstring).  No algorithm here: extern "C" around the
// reference's own AudioBuffer, with the classes opened so that the int16 / float pair's storage and valid flags
// (IFChannelBuffer), the resamplers' input buffers and kernel tables (SincResampler) and the band split's
// TwoBandsStates can be read.  For the last run high_pass_filter_impl.cc is included, as hpf_ref_shim.cc does, and
// HighPassFilterImpl::ProcessCaptureAudio's loop over the channels' band 0 calls its Filter on the buffer.
#include <stdint.h>
#include <string.h>

#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#define private public
#include "webrtc/common_audio/resampler/push_sinc_resampler.h"
#include "webrtc/common_audio/resampler/sinc_resampler.h"
#include "webrtc/modules/audio_processing/audio_buffer.h"
#include "webrtc/modules/audio_processing/channel_buffer.h"
#include "webrtc/modules/audio_processing/splitting_filter.h"
#undef private

#include "webrtc/modules/audio_processing/high_pass_filter_impl.cc"

using webrtc::AudioBuffer;
using webrtc::AudioFrame;
using webrtc::AudioProcessing;
using webrtc::Band;
using webrtc::FilterState;
using webrtc::IFChannelBuffer;
using webrtc::PushSincResampler;
using webrtc::SincResampler;
using webrtc::TwoBandsStates;

namespace {
AudioBuffer* AB(void* h) { return (AudioBuffer*)h; }

IFChannelBuffer* pair_of(AudioBuffer* a, int band) {
  if (band < 0) return a->channels_.get();
  return (size_t)band < a->split_channels_.size() ? a->split_channels_[band] : NULL;
}

void frame_for(AudioBuffer* a, AudioFrame* f) {
  f->samples_per_channel_ = a->proc_samples_per_channel_;
  f->num_channels_ = a->num_input_channels_;
}
}  // namespace

extern "C" {

void* ab_ref_create(int in, int cin, int proc, int cproc, int out) { return new AudioBuffer(in, cin, proc, cproc, out); }
void ab_ref_free(void* h) { delete AB(h); }

void ab_ref_deinterleave(void* h, const int16_t* data, int activity) {
  AudioFrame f;
  frame_for(AB(h), &f);
  f.vad_activity_ = (AudioFrame::VADActivity)activity;
  memcpy(f.data_, data, sizeof(int16_t) * f.samples_per_channel_ * f.num_channels_);
  AB(h)->DeinterleaveFrom(&f);
}

// data: what the frame holds before the call, and after it; returns the frame's activity after the call
int ab_ref_interleave(void* h, int16_t* data, int activity_before, int data_changed) {
  AudioFrame f;
  frame_for(AB(h), &f);
  f.vad_activity_ = (AudioFrame::VADActivity)activity_before;
  const size_t bytes = sizeof(int16_t) * f.samples_per_channel_ * f.num_channels_;
  memcpy(f.data_, data, bytes);
  AB(h)->InterleaveTo(&f, data_changed != 0);
  memcpy(data, f.data_, bytes);
  return f.vad_activity_;
}

// planar [channels of the layout][input_samples]; returns keyboard_data() as an offset in floats into planar, -1: NULL
long ab_ref_copy_from(void* h, const float* planar, int layout) {
  AudioBuffer* a = AB(h);
  const int n = a->input_samples_per_channel_;
  const float* ptr[3] = {planar, planar + n, planar + 2 * n};
  a->CopyFrom(ptr, n, (AudioProcessing::ChannelLayout)layout);
  return a->keyboard_data() ? (long)(a->keyboard_data() - planar) : -1;
}

// planar [num_channels()][output_samples]
void ab_ref_copy_to(void* h, float* planar) {
  AudioBuffer* a = AB(h);
  const int n = a->output_samples_per_channel_;
  float* ptr[2] = {planar, planar + n};
  a->CopyTo(n, a->num_channels() == 1 ? AudioProcessing::kMono : AudioProcessing::kStereo, ptr);
}

void ab_ref_split(void* h) { AB(h)->SplitIntoFrequencyBands(); }
void ab_ref_merge(void* h) { AB(h)->MergeFrequencyBands(); }
void ab_ref_copy_low_pass(void* h) { AB(h)->CopyLowPassToReference(); }

// out [Cproc][samples_per_split_channel]; 0: low_pass_reference() is NULL
int ab_ref_low_pass_reference(void* h, int16_t* out) {
  AudioBuffer* a = AB(h);
  const int n = a->samples_per_split_channel();
  for (int c = 0; c < a->num_proc_channels_; ++c) {
    const int16_t* p = a->low_pass_reference(c);
    if (!p) return 0;
    memcpy(out + c * n, p, n * sizeof(int16_t));
  }
  return 1;
}

void ab_ref_mixed(void* h, int16_t* out) {
  AudioBuffer* a = AB(h);
  memcpy(out, a->mixed_low_pass_data(), a->samples_per_split_channel() * sizeof(int16_t));
}

// The accessor of (kind, band): kind 0 int16, 1 const int16, 2 float, 3 const float; band < 0: channels().  With
// write (non-const kinds) the caller's [Cproc][n] is stored through the returned pointers; out receives what they
// point at.  0: the accessor returned NULL.
int ab_ref_view(void* h, int kind, int band, const void* write, void* out) {
  AudioBuffer* a = AB(h);
  const int n = band < 0 ? a->samples_per_channel() : a->samples_per_split_channel();
  const int C = a->num_proc_channels_;
  if (kind < 2) {
    int16_t* const* p = NULL;
    if (kind == 0) p = band < 0 ? a->channels() : a->split_channels((Band)band);
    else p = const_cast<int16_t* const*>(band < 0 ? a->channels_const() : a->split_channels_const((Band)band));
    if (!p) return 0;
    for (int c = 0; c < C; ++c) {
      if (write && kind == 0) memcpy(p[c], (const int16_t*)write + c * n, n * sizeof(int16_t));
      memcpy((int16_t*)out + c * n, p[c], n * sizeof(int16_t));
    }
  } else {
    float* const* p = NULL;
    if (kind == 2) p = band < 0 ? a->channels_f() : a->split_channels_f((Band)band);
    else p = const_cast<float* const*>(band < 0 ? a->channels_const_f() : a->split_channels_const_f((Band)band));
    if (!p) return 0;
    for (int c = 0; c < C; ++c) {
      if (write && kind == 2) memcpy(p[c], (const float*)write + c * n, n * sizeof(float));
      memcpy((float*)out + c * n, p[c], n * sizeof(float));
    }
  }
  return 1;
}

// the pair's storage and flags as they are, no accessor; 0: the buffer has no such band
int ab_ref_raw(void* h, int band, int16_t* i_out, float* f_out, int* ivalid, int* fvalid) {
  IFChannelBuffer* p = pair_of(AB(h), band);
  if (!p) return 0;
  memcpy(i_out, p->ibuf_.data(), p->ibuf_.length() * sizeof(int16_t));
  memcpy(f_out, p->fbuf_.data(), p->fbuf_.length() * sizeof(float));
  *ivalid = p->ivalid_;
  *fvalid = p->fvalid_;
  return 1;
}

void ab_ref_flags(void* h, int* mixed_valid, int* reference_copied) {
  *mixed_valid = AB(h)->mixed_low_pass_valid_;
  *reference_copied = AB(h)->reference_copied_;
}

int ab_ref_num_channels(void* h) { return AB(h)->num_channels(); }
void ab_ref_set_num_channels(void* h, int n) { AB(h)->set_num_channels(n); }
int ab_ref_num_bands(void* h) { return AB(h)->num_bands(); }
int ab_ref_samples_per_channel(void* h) { return AB(h)->samples_per_channel(); }
int ab_ref_samples_per_split_channel(void* h) { return AB(h)->samples_per_split_channel(); }
int ab_ref_samples_per_keyboard_channel(void* h) { return AB(h)->samples_per_keyboard_channel(); }
int ab_ref_activity(void* h) { return AB(h)->activity(); }
void ab_ref_set_activity(void* h, int v) { AB(h)->set_activity((AudioFrame::VADActivity)v); }

// which 0: input_resamplers_[ch], 1: output_resamplers_[ch], 2 / 3: the band split's analysis / synthesis resampler.
// buffer receives input_buffer_ (request frames + 32 floats), kernel the 33 x 32 table; returns the buffer's length,
// 0 when the buffer has no such resampler.
int ab_ref_resampler(void* h, int which, int ch, float* buffer, float* kernel) {
  AudioBuffer* a = AB(h);
  PushSincResampler* r = NULL;
  if (which == 0 && (size_t)ch < a->input_resamplers_.size()) r = a->input_resamplers_[ch];
  if (which == 1 && (size_t)ch < a->output_resamplers_.size()) r = a->output_resamplers_[ch];
  if (which >= 2 && a->splitting_filter_.get() && a->num_bands() == 3)
    r = which == 2 ? a->splitting_filter_->analysis_resamplers_[ch] : a->splitting_filter_->synthesis_resamplers_[ch];
  if (!r) return 0;
  SincResampler* s = r->resampler_.get();
  memcpy(buffer, s->input_buffer_.get(), s->input_buffer_size_ * sizeof(float));
  memcpy(kernel, s->kernel_storage_.get(),
         SincResampler::kKernelSize * (SincResampler::kKernelOffsetCount + 1) * sizeof(float));
  return s->input_buffer_size_;
}

// two_bands_states_[ch], band1_states_[ch], band2_states_[ch]: 3 x (analysis 1, 2, synthesis 1, 2) x 6 words
int ab_ref_split_state(void* h, int ch, int32_t* out) {
  AudioBuffer* a = AB(h);
  if (!a->splitting_filter_.get()) return 0;
  const TwoBandsStates* st[3] = {&a->splitting_filter_->two_bands_states_[ch], &a->splitting_filter_->band1_states_[ch],
                                 &a->splitting_filter_->band2_states_[ch]};
  for (int k = 0; k < 3; ++k) {
    memcpy(out + k * 24, st[k]->analysis_state1, 6 * sizeof(int32_t));
    memcpy(out + k * 24 + 6, st[k]->analysis_state2, 6 * sizeof(int32_t));
    memcpy(out + k * 24 + 12, st[k]->synthesis_state1, 6 * sizeof(int32_t));
    memcpy(out + k * 24 + 18, st[k]->synthesis_state2, 6 * sizeof(int32_t));
  }
  return 1;
}

// HighPassFilterImpl: one FilterState per channel, InitializeHandle's InitializeFilter, and ProcessCaptureAudio's loop
void* ab_ref_hpf_create(int sample_rate_hz, int channels) {
  FilterState* s = new FilterState[channels];
  for (int i = 0; i < channels; ++i) webrtc::InitializeFilter(&s[i], sample_rate_hz);
  return s;
}
void ab_ref_hpf_free(void* s) { delete[] (FilterState*)s; }
void ab_ref_hpf_process(void* s, void* h, int channels) {
  AudioBuffer* audio = AB(h);
  for (int i = 0; i < channels; i++)
    webrtc::Filter(&((FilterState*)s)[i], audio->split_bands(i)[webrtc::kBand0To8kHz], audio->samples_per_split_channel());
}
void ab_ref_hpf_state(void* s, int ch, int16_t* out) {
  const FilterState* f = &((const FilterState*)s)[ch];
  for (int i = 0; i < 4; ++i) out[i] = f->y[i];
  out[4] = f->x[0];
  out[5] = f->x[1];
}
}
