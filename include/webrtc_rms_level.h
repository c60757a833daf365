/*
 * webrtc_rms_level.h -- the reference's webrtc::RMSLevel
 * (WebRtc_AMP_Port/webrtc/modules/audio_processing/rms_level.h, rms_level.cc) as a header-only C++ layer over the
 * C-ABI of asp_level.h.  Same method names, return values and kMinLevel; an object is a batch of one stream on
 * the GPU.  Without a HIP device the object has no batch: Process and ProcessMuted do nothing and RMS returns
 * kMinLevel (the reference's methods have no way to report a failure); ok() tells.  There is no CPU path.
 */
#ifndef ASP_WEBRTC_RMS_LEVEL_H_
#define ASP_WEBRTC_RMS_LEVEL_H_

#include <stdint.h>

#include "asp_level.h"

namespace webrtc {

class RMSLevel {
 public:
  static const int kMinLevel = ASP_LEVEL_MIN;

  /* Extension: the GPU (the reference's constructor takes no argument). */
  explicit RMSLevel(int device = 0) : batch_(0) {
    if (AspLevelBatch_Create(&batch_, 1, device) != ASP_OK) batch_ = 0;
  }
  ~RMSLevel() {
    if (batch_) AspLevelBatch_Free(batch_);
  }

  /* Extension: false when no batch could be created. */
  bool ok() const { return batch_ != 0; }

  // Can be called to reset internal states, but is not required during normal operation.
  void Reset() {
    if (batch_) AspLevelBatch_Reset(batch_);
  }

  // Pass each chunk of audio to Process() to accumulate the level.
  void Process(const int16_t* data, int length) {
    // RMSLevel takes any length; the batch takes ASP_LEVEL_MAX_SAMPLES a call
    for (int i = 0; batch_ && i < length; i += ASP_LEVEL_MAX_SAMPLES) {
      const int n = length - i < ASP_LEVEL_MAX_SAMPLES ? length - i : ASP_LEVEL_MAX_SAMPLES;
      AspLevelBatch_Process(batch_, data + i, 1, 1, n, ASP_MEM_HOST);
    }
  }

  // If all samples with the given |length| have a magnitude of zero, this is a shortcut to avoid some computation.
  void ProcessMuted(int length) {
    if (batch_) AspLevelBatch_ProcessMuted(batch_, length);
  }

  // Computes the RMS level over all data passed to Process() since the last call to RMS(). The returned value is
  // positive but should be interpreted as negative as per the RFC. It is constrained to [0, 127].
  int RMS() {
    int32_t level = kMinLevel;
    if (batch_ && AspLevelBatch_RMS(batch_, &level) != ASP_OK) level = kMinLevel;
    return level;
  }

 private:
  RMSLevel(const RMSLevel&);
  RMSLevel& operator=(const RMSLevel&);

  AspLevelBatch* batch_;
};

}  // namespace webrtc

#endif /* ASP_WEBRTC_RMS_LEVEL_H_ */
