/*
 * webrtc_transient_suppressor.h -- the reference's webrtc::TransientSuppressor
 * (WebRtc_AMP_Port/webrtc/modules/audio_processing/transient/transient_suppressor.h) as a header-only C++ layer
 * over the C-ABI of asp_ts.h.  Same method names, signatures and return values; an object is a batch of one
 * stream on the GPU.  Without a HIP device Initialize returns -1: there is no CPU path.
 *
 * One difference: with detection_data NULL the reference reads detection_length samples from the newest
 * chunk of in_buffer_, past its end when the detection rate is above the sample rate; here that call returns -1.
 */
#ifndef ASP_WEBRTC_TRANSIENT_SUPPRESSOR_H_
#define ASP_WEBRTC_TRANSIENT_SUPPRESSOR_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ts.h"

namespace webrtc {

class TransientSuppressor {
 public:
  TransientSuppressor() : batch_(0), device_(0) {}
  ~TransientSuppressor() {
    if (batch_) AspTsBatch_Free(batch_);
  }

  // the GPU the next Initialize creates the instance on (default 0)
  void set_device(int device) { device_ = device; }

  int Initialize(int sample_rate_hz, int detection_rate_hz, int num_channels) {
    if (!batch_ && AspTsBatch_Create(&batch_, 1, device_) != 0) {
      batch_ = 0;
      return -1;
    }
    return AspTsBatch_Initialize(batch_, sample_rate_hz, detection_rate_hz, num_channels) == 0 ? 0 : -1;
  }

  // Processes a |data| chunk (interleaved by channel planes: [num_channels][data_length]) and returns it with
  // keystrokes suppressed, delayed by analysis_length - data_length samples.  Host memory.
  int Suppress(float* data, size_t data_length, int num_channels, const float* detection_data,
               size_t detection_length, const float* reference_data, size_t reference_length,
               float voice_probability, bool key_pressed) {
    if (!batch_) return -1;
    const uint8_t key = key_pressed ? 1 : 0;
    return AspTsBatch_Suppress(batch_, data, data_length, num_channels, detection_data, detection_length,
                               reference_data, reference_length, 0, &voice_probability, &key, 0, ASP_MEM_HOST) == 0
               ? 0
               : -1;
  }

 private:
  TransientSuppressor(const TransientSuppressor&);
  TransientSuppressor& operator=(const TransientSuppressor&);
  AspTsBatch* batch_;
  int device_;
};

}  // namespace webrtc

#endif  // ASP_WEBRTC_TRANSIENT_SUPPRESSOR_H_
