/*
 * asp_resampler.h -- C-ABI of the MI355X batched fixed-point resampler: the reference's webrtc::Resampler
 * (WebRtc_AMP_Port/webrtc/common_audio/resampler/resampler.cc over the spl primitives resample_by_2.c,
 * resample_48khz.c, resample.c, resample_by_2_internal.c, resample_fractional.c).  int16 in / int16 out,
 * integer arithmetic, bit-exact.  (asp_resample.h is another thing: the float PushSincResampler of the
 * band split.)
 *
 * N independent streams per call, every stream's filter state resident in HBM; one rate pair per batch.
 * include/webrtc_resampler.h puts the reference's own class over a batch of one stream.
 * No CPU fallback: without a HIP device Create fails.
 */
#ifndef ASP_RESAMPLER_H_
#define ASP_RESAMPLER_H_
#include <stddef.h>
#include <stdint.h>
#include "asp_ns.h" /* ASP_OK / ASP_ERR_*, ASP_MEM_HOST / ASP_MEM_DEVICE */
#ifdef __cplusplus
extern "C" {
#endif
typedef struct AspResamplerBatch AspResamplerBatch;
/* One channel of one stream.  mode: the reference's ResamplerMode (0 = 1To1 ... 20 = 11To8), -1 after a
 * failed Reset.  stage[k]: state(k+1)_ of the reference as int32 words in its struct's field order (a by-2
 * stage: 8 words; WebRtcSpl_State16khzTo48khz: S_16_32, S_32_24, S_24_48; ...48khzTo16khz: S_48_48[16],
 * S_48_32, S_32_16; ...22khzTo16khz: S_22_44, S_44_32, S_32_16; ...16khzTo22khz: S_16_32, S_32_22;
 * ...22khzTo8khz: S_22_22[16], S_22_16, S_16_8; ...8khzTo22khz: S_8_16, S_16_11, S_11_22); unused words
 * are 0. */
typedef struct AspResamplerState {
  int32_t mode;
  int32_t in_freq_khz, out_freq_khz;
  int32_t stage[3][32];
} AspResamplerState;
int AspResamplerBatch_Create(AspResamplerBatch** out, int num_streams, int device);
int AspResamplerBatch_Free(AspResamplerBatch* b);
int AspResamplerBatch_num_streams(const AspResamplerBatch* b);
/* Resampler::Reset for every stream: 0, or -1 for a ratio outside the reference's 21 modes (after which
 * every Push returns -1, as with kResamplerInvalid).  channels 1: kResamplerSynchronous; 2:
 * kResamplerSynchronousStereo (interleaved in and out, each channel filtered with its own state). */
int AspResamplerBatch_Reset(AspResamplerBatch* b, int in_freq, int out_freq, int channels);
/* Resets only when in_freq / 1000, out_freq / 1000 or channels differ from the last Reset. */
int AspResamplerBatch_ResetIfNeeded(AspResamplerBatch* b, int in_freq, int out_freq, int channels);
/* Zeroes one stream's filter state (every channel) inside a running batch. */
int AspResamplerBatch_ResetStream(AspResamplerBatch* b, int stream);
/* The outLen a Push of length_in samples would report, or -1 where the reference rejects the length. */
int AspResamplerBatch_OutLength(const AspResamplerBatch* b, int length_in);
/* Resampler::Push for every stream.  in [num_streams][length_in], out [num_streams][*out_len] (dense);
 * max_len is per stream.  Returns 0, or -1 where the reference returns -1 (block length, max_len, no valid
 * Reset); a rejected Push leaves the state untouched (the reference's 3To2 runs its first stage before it
 * rejects a length that is no multiple of 240).  Two more departures, both refusals with -1: mode 1To1
 * checks max_len as every other mode does (the reference copies without looking), and an odd length_in with
 * two channels (the reference reads one sample past the input).  in and out must not overlap: an overlap is
 * refused with ASP_ERR_PARAM.  mem: ASP_MEM_*; the call returns when the output is complete. */
int AspResamplerBatch_Push(AspResamplerBatch* b, const int16_t* in, int length_in, int16_t* out, int max_len,
                           int* out_len, int mem);
/* num_frames consecutive Pushes in one launch: in [num_frames][num_streams][length_in],
 * out [num_frames][num_streams][OutLength(length_in)].  Bit-equal to num_frames single calls. */
int AspResamplerBatch_PushFrames(AspResamplerBatch* b, const int16_t* in, int length_in, int num_frames,
                                 int16_t* out, int mem);
int AspResamplerBatch_ExportState(AspResamplerBatch* b, int stream, int channel, AspResamplerState* out);
/* in->mode must be the batch's mode (one mode per batch). */
int AspResamplerBatch_ImportState(AspResamplerBatch* b, int stream, int channel, const AspResamplerState* in);
int AspResamplerBatch_SetStream(AspResamplerBatch* b, void* hip_stream); /* NULL: back to the batch's own stream */
int AspResamplerBatch_Synchronize(AspResamplerBatch* b);
size_t AspResampler_state_size(void); /* sizeof(AspResamplerState) */
#ifdef __cplusplus
}
#endif
#endif /* ASP_RESAMPLER_H_ */
