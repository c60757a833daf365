// splrs_ref_shim.cc -- extern "C" access to the reference's webrtc::Resampler for
// tests/golden/make_splrs_golden.py (the compile line is in that script's docstring).  No algorithm here:
// create / reset / push, and a copy of the words of state1_ .. state3_ (private members, opened below).
#include <stdint.h>
#include <string.h>

#define private public
#include "webrtc/common_audio/resampler/include/resampler.h"
#undef private

using webrtc::Resampler;
using webrtc::ResamplerType;

extern "C" {
void* splrs_ref_create(void) { return new Resampler(); }
void splrs_ref_free(void* h) { delete (Resampler*)h; }
int splrs_ref_reset(void* h, int in_freq, int out_freq, int type) {
  return ((Resampler*)h)->Reset(in_freq, out_freq, (ResamplerType)type);
}
int splrs_ref_reset_if_needed(void* h, int in_freq, int out_freq, int type) {
  return ((Resampler*)h)->ResetIfNeeded(in_freq, out_freq, (ResamplerType)type);
}
int splrs_ref_push(void* h, const int16_t* in, int length_in, int16_t* out, int max_len, int* out_len) {
  return ((Resampler*)h)->Push(in, length_in, out, max_len, *out_len);
}
int splrs_ref_mode(void* h) { return (int)((Resampler*)h)->my_mode_; }
// which: 0 the instance itself, 1 slave_left_, 2 slave_right_; k: 0..2; words: what Reset allocated for it
int splrs_ref_state(void* h, int which, int k, int words, int32_t* out) {
  Resampler* r = (Resampler*)h;
  if (which == 1) r = r->slave_left_;
  if (which == 2) r = r->slave_right_;
  if (!r) return -1;
  void* p = k == 0 ? r->state1_ : k == 1 ? r->state2_ : r->state3_;
  if (!p) return -1;
  memcpy(out, p, words * sizeof(int32_t));
  return 0;
}
}
