// ts_ref_shim.cc -- extern "C" access to the reference's webrtc::TransientSuppressor for
// tests/golden/make_ts_golden.py (the compile line is in that script's docstring).  No algorithm here:
// create / initialize / suppress, copies of private members (opened below), and the stub of
// webrtc::LogMessage that the suppressor's two LOG lines link against.
#include <stdint.h>
#include <string.h>

#include <deque>
#include <queue>
#include <sstream>

#define private public
#include "webrtc/common_audio/fir_filter_sse.h"
#include "webrtc/modules/audio_processing/transient/moving_moments.h"
#include "webrtc/modules/audio_processing/transient/transient_detector.h"
#include "webrtc/modules/audio_processing/transient/transient_suppressor.h"
#include "webrtc/modules/audio_processing/transient/wpd_node.h"
#include "webrtc/modules/audio_processing/transient/wpd_tree.h"
#undef private
#include "webrtc/system_wrappers/interface/logging.h"

namespace webrtc {
LogMessage::LogMessage(const char*, int, LoggingSeverity) {}
LogMessage::~LogMessage() {}
bool LogMessage::Loggable(LoggingSeverity) { return false; }
}  // namespace webrtc

using webrtc::TransientSuppressor;

namespace {
struct OpenQueue : std::queue<float> {
  static std::deque<float> std::queue<float>::*container() { return &OpenQueue::c; }
};
}  // namespace

extern "C" {
void* ts_ref_create(void) { return new TransientSuppressor(); }
void ts_ref_free(void* h) { delete (TransientSuppressor*)h; }
int ts_ref_initialize(void* h, int rate, int det_rate, int channels) {
  return ((TransientSuppressor*)h)->Initialize(rate, det_rate, channels);
}
int ts_ref_suppress(void* h, float* data, size_t data_length, int num_channels, const float* detection_data,
                    size_t detection_length, const float* reference_data, size_t reference_length,
                    float voice_probability, int key_pressed) {
  return ((TransientSuppressor*)h)
      ->Suppress(data, data_length, num_channels, detection_data, detection_length, reference_data, reference_length,
                 voice_probability, key_pressed != 0);
}
// i[0..8]: keypress_counter_, chunks_since_keypress_, detection_enabled_, suppression_enabled_,
// use_hard_restoration_, chunks_since_voice_change_, seed_, using_reference_, chunks_at_startup_left_to_delete_;
// f[0..1]: detector_smoothed_, reference_energy_; f[2..4]: previous_results_
void ts_ref_scalars(void* h, int64_t* i, float* f) {
  TransientSuppressor* t = (TransientSuppressor*)h;
  i[0] = t->keypress_counter_;
  i[1] = t->chunks_since_keypress_;
  i[2] = t->detection_enabled_;
  i[3] = t->suppression_enabled_;
  i[4] = t->use_hard_restoration_;
  i[5] = t->chunks_since_voice_change_;
  i[6] = t->seed_;
  i[7] = t->using_reference_;
  i[8] = t->detector_->chunks_at_startup_left_to_delete_;
  f[0] = t->detector_smoothed_;
  f[1] = t->detector_->reference_energy_;
  for (int k = 0; k < 3; ++k) f[2 + k] = t->detector_->previous_results_[k];
}
// which: 0 in_buffer_, 1 out_buffer_, 2 spectral_mean_, 3 window_, 4 wfft_, 5 mean_factor_, 6 magnitudes_;
// returns the count
int ts_ref_array(void* h, int which, float* out) {
  TransientSuppressor* t = (TransientSuppressor*)h;
  const size_t n = t->analysis_length_, b = t->complex_analysis_length_, c = t->num_channels_;
  const float* p = which == 0 ? t->in_buffer_.get() : which == 1 ? t->out_buffer_.get()
                 : which == 2 ? t->spectral_mean_.get() : which == 3 ? t->window_
                 : which == 4 ? t->wfft_.get() : which == 5 ? t->mean_factor_.get() : t->magnitudes_.get();
  const size_t len = which < 2 ? n * c : which == 2 ? b * c : which == 3 ? n : which == 4 ? b - 1 : b;
  memcpy(out, p, len * sizeof(float));
  return (int)len;
}
// the FIR state (15 samples) of tree node 2..15 (1-based, as WPDTree numbers them)
void ts_ref_node_state(void* h, int node, float* out) {
  webrtc::WPDNode* n = ((TransientSuppressor*)h)->detector_->wpd_tree_->nodes_[node].get();
  webrtc::FIRFilterSSE2* f = (webrtc::FIRFilterSSE2*)n->filter_.get();
  memcpy(out, f->state_.get(), 15 * sizeof(float));
}
// leaf 0..7: the queue oldest first (returns its length), sum_, sum_of_squares_, last_first / last_second
int ts_ref_moments(void* h, int leaf, float* queue, float* sums) {
  webrtc::TransientDetector* d = ((TransientSuppressor*)h)->detector_.get();
  webrtc::MovingMoments* m = d->moving_moments_[leaf].get();
  const std::deque<float>& q = m->queue_.*OpenQueue::container();
  for (size_t k = 0; k < q.size(); ++k) queue[k] = q[k];
  sums[0] = m->sum_;
  sums[1] = m->sum_of_squares_;
  sums[2] = d->last_first_moment_[leaf];
  sums[3] = d->last_second_moment_[leaf];
  return (int)q.size();
}
}
