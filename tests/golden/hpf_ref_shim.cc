// hpf_ref_shim.cc -- access code for tests/golden/make_hpf_golden.py, compiled against the reference in the build
// container only (the compile line is in the generator's docstring).  No algorithm here: the reference's
// high_pass_filter_impl.cc is included so that the InitializeFilter / Filter of its anonymous namespace can be
// called from this translation unit, and rms_level.h is opened so that RMSLevel's two members can be read.
#include <stdint.h>

#define private public
#include "webrtc/modules/audio_processing/rms_level.h"
#undef private

#include "webrtc/modules/audio_processing/high_pass_filter_impl.cc"

#include "webrtc/common_audio/include/audio_util.h"

using webrtc::FilterState;
using webrtc::RMSLevel;

extern "C" {

void* hpf_ref_create(int sample_rate_hz) {
  FilterState* s = new FilterState;
  webrtc::InitializeFilter(s, sample_rate_hz);
  return s;
}
void hpf_ref_free(void* h) { delete (FilterState*)h; }
int hpf_ref_filter(void* h, int16_t* data, int length) { return webrtc::Filter((FilterState*)h, data, length); }
// y[0..3], x[0..1]
void hpf_ref_state(void* h, int16_t* out) {
  const FilterState* s = (const FilterState*)h;
  for (int i = 0; i < 4; ++i) out[i] = s->y[i];
  out[4] = s->x[0];
  out[5] = s->x[1];
}
// 0: kFilterCoefficients8kHz, 1: kFilterCoefficients
int hpf_ref_coeff_set(void* h) { return ((const FilterState*)h)->ba == webrtc::kFilterCoefficients8kHz ? 0 : 1; }

// the array form of FloatS16ToS16 (audio_util.cc)
void hpf_ref_float_s16_to_s16(const float* src, int n, int16_t* dst) { webrtc::FloatS16ToS16(src, (size_t)n, dst); }

void* level_ref_create(void) { return new RMSLevel; }
void level_ref_free(void* h) { delete (RMSLevel*)h; }
void level_ref_reset(void* h) { ((RMSLevel*)h)->Reset(); }
void level_ref_process(void* h, const int16_t* data, int length) { ((RMSLevel*)h)->Process(data, length); }
void level_ref_muted(void* h, int length) { ((RMSLevel*)h)->ProcessMuted(length); }
int level_ref_rms(void* h) { return ((RMSLevel*)h)->RMS(); }
void level_ref_state(void* h, float* sum_square, int* sample_count) {
  *sum_square = ((RMSLevel*)h)->sum_square_;
  *sample_count = ((RMSLevel*)h)->sample_count_;
}
}
