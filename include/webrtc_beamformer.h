/*
 * webrtc_beamformer.h -- the reference's webrtc::Beamformer
 * (WebRtc_AMP_Port/webrtc/modules/audio_processing/beamformer/beamformer.h) as a header-only C++ layer over the
 * C-ABI of asp_bf.h.  Same constructor and method names and signatures; an object is a batch of one stream on the
 * GPU.  Host memory; output[0] may be input[0].
 *
 * Where the reference CHECKs (and aborts) -- a geometry that is not a uniform linear array, a channel or frame
 * count other than the initialised one -- and where this library refuses a call (a band rate other than 16 kHz,
 * a chunk other than 10 ms, no HIP device: there is no CPU path), the call does nothing and status() returns the
 * negative ASP_ERR_* code; AspNs_last_error() has the text.
 */
#ifndef ASP_WEBRTC_BEAMFORMER_H_
#define ASP_WEBRTC_BEAMFORMER_H_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "asp_bf.h"

namespace webrtc {

#ifndef ASP_WEBRTC_POINT_DEFINED
#define ASP_WEBRTC_POINT_DEFINED
// modules/audio_processing/include/audio_processing.h
struct Point {
  Point(float x, float y, float z) {
    c[0] = x;
    c[1] = y;
    c[2] = z;
  }
  float c[3];
};
#endif

class Beamformer {
 public:
  explicit Beamformer(const std::vector<Point>& array_geometry)
      : batch_(0), device_(0), status_(ASP_ERR_STATE), target_(0), num_mics_((int)array_geometry.size()) {
    for (size_t i = 0; i < array_geometry.size(); ++i)
      for (int k = 0; k < 3; ++k) xyz_.push_back(array_geometry[i].c[k]);
  }
  virtual ~Beamformer() {
    if (batch_) AspBfBatch_Free(batch_);
  }

  // the GPU the next Initialize creates the instance on (default 0)
  void set_device(int device) { device_ = device; }
  // 0 after a successful Initialize / ProcessChunk, else the ASP_ERR_* code of the last refused call
  int status() const { return status_; }

  // Sample rate corresponds to the lower band.  Needs to be called before the Beamformer can be used.
  virtual void Initialize(int chunk_size_ms, int sample_rate_hz) {
    target_ = 0;
    if (!batch_ && (status_ = AspBfBatch_Create(&batch_, 1, device_)) != 0) {
      batch_ = 0;
      return;
    }
    status_ = AspBfBatch_Initialize(batch_, num_mics_, xyz_.empty() ? 0 : &xyz_[0], chunk_size_ms, sample_rate_hz);
  }

  // Process one time-domain chunk of audio: input[num_input_channels][num_frames_per_band], the higher half of
  // the spectrum as high_pass_split_input (or NULL), one channel out in output[0] (and high_pass_split_output[0]).
  virtual void ProcessChunk(const float* const* input, const float* const* high_pass_split_input,
                            int num_input_channels, int num_frames_per_band, float* const* output,
                            float* const* high_pass_split_output) {
    if (!batch_ || AspBfBatch_state_floats(batch_) < 0) {
      status_ = ASP_ERR_STATE;
      return;
    }
    if (num_input_channels != num_mics_ || num_frames_per_band != ASP_BF_CHUNK || !input || !output ||
        (high_pass_split_input && !high_pass_split_output)) {
      status_ = ASP_ERR_PARAM;
      return;
    }
    const size_t n = (size_t)num_mics_ * ASP_BF_CHUNK;
    in_.resize(2 * n);
    for (int c = 0; c < num_mics_; ++c) {
      memcpy(&in_[(size_t)c * ASP_BF_CHUNK], input[c], sizeof(float) * ASP_BF_CHUNK);
      if (high_pass_split_input)
        memcpy(&in_[n + (size_t)c * ASP_BF_CHUNK], high_pass_split_input[c], sizeof(float) * ASP_BF_CHUNK);
    }
    float out[2][ASP_BF_CHUNK];
    uint8_t target = 0;
    status_ = AspBfBatch_ProcessChunk(batch_, &in_[0], high_pass_split_input ? &in_[n] : 0, out[0],
                                      high_pass_split_input ? out[1] : 0, &target, ASP_MEM_HOST);
    if (status_ != 0) return;
    target_ = target;
    memcpy(output[0], out[0], sizeof out[0]);
    if (high_pass_split_input) memcpy(high_pass_split_output[0], out[1], sizeof out[1]);
  }

  // true when the target signal was present in the last processed chunk's last block
  virtual bool is_target_present() { return target_ != 0; }

 private:
  Beamformer(const Beamformer&);
  Beamformer& operator=(const Beamformer&);
  AspBfBatch* batch_;
  int device_, status_, target_, num_mics_;
  std::vector<float> xyz_, in_;
};

}  // namespace webrtc

#endif  // ASP_WEBRTC_BEAMFORMER_H_
