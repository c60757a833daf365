/*
 * webrtc_resampler.h -- the reference's webrtc::Resampler
 * (WebRtc_AMP_Port/webrtc/common_audio/resampler/include/resampler.h, resampler.cc) as a header-only C++
 * layer over the C-ABI of asp_resampler.h.  Same enum values, constructors, method names and return
 * values; a handle is a batch of one stream on the GPU.  Without a HIP device Reset returns -1 and the
 * object stays kResamplerInvalid: there is no CPU path.
 *
 * Insert / Pull (the asynchronous interface) are declared and return -1.  The reference's own versions
 * cannot be pinned to a behaviour: Insert resamples from in_buffer_, which is NULL on its direct path
 * (resampler.cc:1048), and Pull copies desiredLen * sizeof(int32_t) bytes of int16 data (:1068).
 */
#ifndef ASP_WEBRTC_RESAMPLER_H_
#define ASP_WEBRTC_RESAMPLER_H_

#include <stdint.h>

#include "asp_resampler.h"

namespace webrtc {

enum ResamplerType {
  // 4 MSB = number of channels, 4 LSB = synchronous or asynchronous
  kResamplerSynchronous = 0x10,
  kResamplerAsynchronous = 0x11,
  kResamplerSynchronousStereo = 0x20,
  kResamplerAsynchronousStereo = 0x21,
  kResamplerInvalid = 0xff
};

enum ResamplerMode {
  kResamplerMode1To1,
  kResamplerMode1To2,
  kResamplerMode1To3,
  kResamplerMode1To4,
  kResamplerMode1To6,
  kResamplerMode1To12,
  kResamplerMode2To3,
  kResamplerMode2To11,
  kResamplerMode4To11,
  kResamplerMode8To11,
  kResamplerMode11To16,
  kResamplerMode11To32,
  kResamplerMode2To1,
  kResamplerMode3To1,
  kResamplerMode4To1,
  kResamplerMode6To1,
  kResamplerMode12To1,
  kResamplerMode3To2,
  kResamplerMode11To2,
  kResamplerMode11To4,
  kResamplerMode11To8
};

class Resampler {
 public:
  Resampler() : batch_(0), device_(0), my_in_frequency_khz_(0), my_out_frequency_khz_(0), my_type_(kResamplerInvalid) {}
  Resampler(int inFreq, int outFreq, ResamplerType type)
      : batch_(0), device_(0), my_in_frequency_khz_(0), my_out_frequency_khz_(0), my_type_(kResamplerInvalid) {
    Reset(inFreq, outFreq, type);
  }
  ~Resampler() {
    if (batch_) AspResamplerBatch_Free(batch_);
  }

  /* Extension: choose the GPU before the first Reset (default 0). */
  void setDevice(int device) { device_ = device; }

  // Reset all states
  int Reset(int inFreq, int outFreq, ResamplerType type) {
    my_type_ = type;
    my_in_frequency_khz_ = inFreq / 1000;
    my_out_frequency_khz_ = outFreq / 1000;
    if (!batch_ && AspResamplerBatch_Create(&batch_, 1, device_) != ASP_OK) batch_ = 0;
    const int channels = (type & 0xf0) == 0x20 ? 2 : 1;
    if (!batch_ || AspResamplerBatch_Reset(batch_, inFreq, outFreq, channels) != 0) {
      my_type_ = kResamplerInvalid;
      return -1;
    }
    return 0;
  }

  // Reset all states if any parameter has changed
  int ResetIfNeeded(int inFreq, int outFreq, ResamplerType type) {
    if (inFreq / 1000 != my_in_frequency_khz_ || outFreq / 1000 != my_out_frequency_khz_ || type != my_type_)
      return Reset(inFreq, outFreq, type);
    return 0;
  }

  // Synchronous resampling, all output samples are written to samplesOut (which must not overlap samplesIn)
  int Push(const int16_t* samplesIn, int lengthIn, int16_t* samplesOut, int maxLen, int& outLen) {
    if (my_type_ & 0x0f) return -1;  // asynchronous, or invalid
    int n = 0;
    if (AspResamplerBatch_Push(batch_, samplesIn, lengthIn, samplesOut, maxLen, &n, ASP_MEM_HOST) != 0) return -1;
    outLen = n;
    return 0;
  }

  // Asynchronous resampling: not pinned by the reference (see the head of this file)
  int Insert(int16_t* /*samplesIn*/, int /*lengthIn*/) { return -1; }
  int Pull(int16_t* /*samplesOut*/, int /*desiredLen*/, int& /*outLen*/) { return -1; }

 private:
  Resampler(const Resampler&);
  Resampler& operator=(const Resampler&);

  AspResamplerBatch* batch_;
  int device_;
  int my_in_frequency_khz_;
  int my_out_frequency_khz_;
  ResamplerType my_type_;
};

}  // namespace webrtc

#endif /* ASP_WEBRTC_RESAMPLER_H_ */
