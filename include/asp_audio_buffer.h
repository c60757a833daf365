/* asp_audio_buffer.h -- batched WebRTC AudioBuffer on the GPU: the capture frame buffer of the audio processing
 * module (modules/audio_processing/audio_buffer.cc, channel_buffer.cc) for num_streams independent buffers of one
 * geometry, bit-exact with the reference built for x86-64.  It turns what a caller holds (an
 * interleaved int16 frame, or planar float channels, at its own rate and channel count) into what the stages consume
 * (per-channel data with paired int16 / FloatS16 views, 16 kHz bands at 32 / 48 kHz, a mixed low-pass channel, a
 * low-pass reference copy) and back, without leaving the device between two stages.
 *
 * All audio storage is device memory owned by the batch.  What the reference keeps per buffer but which depends
 * only on the call sequence lives once per batch on the host: the valid flags of the int16 / float pairs
 * (IFChannelBuffer), mixed_low_pass_valid_, reference_copied_, num_channels_, and the resamplers' positions.
 *
 * Views.  A view call returns a device address of [S][Cproc][n] (n = proc_samples for the full band,
 * samples_per_split_channel for a band) and does what its reference accessor does: a stale side is refreshed first
 * (one launch on the batch's stream; none when nothing is stale), and a non-const accessor marks the other side
 * stale and the mixed low pass invalid.  The address is what the other batches of this library take with
 * ASP_MEM_DEVICE (one frame, C = Cproc); run them on the same HIP stream (AspAudioBufferBatch_SetStream).  NULL is
 * a band the buffer does not have, or an error (AspNs_last_error() has the text then).
 *
 * Callers' arrays: `mem` says where they live, ASP_MEM_HOST (copied in and out, the call returns when done) or
 * ASP_MEM_DEVICE (the call returns once its launch is queued; 16-byte aligned).  Activity values are always host
 * memory.  Return values: 0, or ASP_ERR_* (asp_ns.h).  There is no CPU path.
 *
 * There is no class mirror of webrtc::AudioBuffer: its accessors hand out host pointers into its own storage for
 * the caller to write through, which device-resident storage cannot honour. */
#ifndef ASP_AUDIO_BUFFER_H_
#define ASP_AUDIO_BUFFER_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h"

#ifdef __cplusplus
extern "C" {
#endif

/* AudioProcessing::ChannelLayout */
#define ASP_AB_MONO 0
#define ASP_AB_STEREO 1
#define ASP_AB_MONO_AND_KEYBOARD 2
#define ASP_AB_STEREO_AND_KEYBOARD 3

/* AudioFrame::VADActivity */
#define ASP_AB_VAD_ACTIVE 0
#define ASP_AB_VAD_PASSIVE 1
#define ASP_AB_VAD_UNKNOWN 2

/* what AspAudioBufferBatch_Read copies */
#define ASP_AB_READ_I16 0       /* int16 [S][Cproc][n] of the full band (band < 0) or a band */
#define ASP_AB_READ_F32 1       /* float, the same */
#define ASP_AB_READ_MIXED 2     /* int16 [S][samples_per_split_channel], the mixed low pass as last computed */
#define ASP_AB_READ_REFERENCE 3 /* int16 [S][Cproc][samples_per_split_channel], the low-pass reference copy */

#define ASP_AB_MAX_BANDS 3

typedef struct AspAudioBufferBatch AspAudioBufferBatch;

/* AudioBuffer(input_samples, num_input_channels, proc_samples, num_proc_channels, output_samples) for every stream.
 * ASP_ERR_PARAM: num_input_channels not 1 or 2, num_proc_channels < 1 or > num_input_channels, input_samples or
 * output_samples not one of 80 / 160 / 320 / 441 / 480, proc_samples not one of 80 / 160 / 320 / 480. */
int AspAudioBufferBatch_Create(AspAudioBufferBatch** out, int num_streams, int input_samples, int num_input_channels,
                               int proc_samples, int num_proc_channels, int output_samples, int device);
int AspAudioBufferBatch_Free(AspAudioBufferBatch* b);
int AspAudioBufferBatch_num_streams(const AspAudioBufferBatch* b);

/* ---- loaders and unloaders ---- */
/* frames [S][input_samples * Cin] interleaved; activity [S] (host) or NULL (every stream's becomes that of a new
 * AudioFrame, unknown).  Needs proc_samples == input_samples.  Stereo to mono is (a + b) / 2 in int. */
int AspAudioBufferBatch_DeinterleaveFrom(AspAudioBufferBatch* b, const int16_t* frames, const int32_t* activity, int mem);
/* frames [S][proc_samples * Cin]; activity [S] (host) or NULL.  data_changed == 0 writes the activity only.  Needs
 * output_samples == proc_samples and num_channels == Cin. */
int AspAudioBufferBatch_InterleaveTo(AspAudioBufferBatch* b, int16_t* frames, int32_t* activity, int data_changed, int mem);
/* data [S][Cin (+ 1 with a keyboard layout)][input_samples] float in [-1, 1]: downmix (l + r) / 2, resampler to the
 * processing rate, FloatToFloatS16 into the float view.  The keyboard channel is remembered by address. */
int AspAudioBufferBatch_CopyFrom(AspAudioBufferBatch* b, const float* data, int layout, int mem);
/* data [S][num_channels][output_samples]: FloatS16ToFloat, resampler to the output rate. */
int AspAudioBufferBatch_CopyTo(AspAudioBufferBatch* b, float* data, int mem);

/* ---- bands ---- */
/* SplittingFilter::Analysis / Synthesis with the reference's view traffic; ASP_ERR_PARAM on a buffer without bands
 * (proc_samples 80 or 160). */
int AspAudioBufferBatch_SplitIntoFrequencyBands(AspAudioBufferBatch* b);
int AspAudioBufferBatch_MergeFrequencyBands(AspAudioBufferBatch* b);
int AspAudioBufferBatch_CopyLowPassToReference(AspAudioBufferBatch* b);
/* [S][Cproc][samples_per_split_channel]; NULL before CopyLowPassToReference (and after every loader) */
const int16_t* AspAudioBufferBatch_low_pass_reference(AspAudioBufferBatch* b);
/* [S][samples_per_split_channel]: band 0 itself for one channel; for two the int16 (a + b) / 2 of the two band-0
 * channels, cached until a non-const accessor runs */
const int16_t* AspAudioBufferBatch_mixed_low_pass_data(AspAudioBufferBatch* b);

/* ---- views ---- */
int16_t* AspAudioBufferBatch_channels(AspAudioBufferBatch* b);
const int16_t* AspAudioBufferBatch_channels_const(AspAudioBufferBatch* b);
float* AspAudioBufferBatch_channels_f(AspAudioBufferBatch* b);
const float* AspAudioBufferBatch_channels_const_f(AspAudioBufferBatch* b);
/* band 0 of a buffer without bands is the full band; a band the buffer does not have is NULL */
int16_t* AspAudioBufferBatch_split_channels(AspAudioBufferBatch* b, int band);
const int16_t* AspAudioBufferBatch_split_channels_const(AspAudioBufferBatch* b, int band);
float* AspAudioBufferBatch_split_channels_f(AspAudioBufferBatch* b, int band);
const float* AspAudioBufferBatch_split_channels_const_f(AspAudioBufferBatch* b, int band);

/* ---- scalars ---- */
int AspAudioBufferBatch_num_channels(const AspAudioBufferBatch* b);
int AspAudioBufferBatch_set_num_channels(AspAudioBufferBatch* b, int num_channels); /* reset by every loader */
int AspAudioBufferBatch_num_bands(const AspAudioBufferBatch* b);
int AspAudioBufferBatch_samples_per_channel(const AspAudioBufferBatch* b);
int AspAudioBufferBatch_samples_per_split_channel(const AspAudioBufferBatch* b);
int AspAudioBufferBatch_samples_per_keyboard_channel(const AspAudioBufferBatch* b);
/* the keyboard channel of stream 0 inside the array the last CopyFrom was given (stream s is s * (Cin + 1) *
 * input_samples floats further); NULL without a keyboard layout */
const float* AspAudioBufferBatch_keyboard_data(const AspAudioBufferBatch* b);
int AspAudioBufferBatch_set_activity(AspAudioBufferBatch* b, int stream, int activity);
int AspAudioBufferBatch_activity(const AspAudioBufferBatch* b, int stream);

/* ---- plumbing ---- */
/* Copies storage to the host as it is: no refresh, no flag changes (tests).  what: ASP_AB_READ_*; band < 0 is the
 * full band.  valid (may be NULL) receives the valid flag of that side, for MIXED / REFERENCE mixed_low_pass_valid_ /
 * reference_copied_. */
int AspAudioBufferBatch_Read(AspAudioBufferBatch* b, int what, int band, void* host_dst, int* valid);
/* the 33 x 32 resampler kernel table built on the host; which 0: input resampler, 1: output.  Returns the number
 * of floats written (1056), 0 when the geometry has no such resampler. */
int AspAudioBufferBatch_kernel_table(const AspAudioBufferBatch* b, int which, float* out, int capacity);
int AspAudioBufferBatch_SetStream(AspAudioBufferBatch* b, void* hip_stream);
int AspAudioBufferBatch_Synchronize(AspAudioBufferBatch* b);

/* Checkpoint of one stream: the batch's record (geometry, flags, resampler positions), then per processing channel
 * the input and output resamplers' buffers and, with bands, the band split's AspSplitState (asp_split.h).  The audio
 * itself is not part of it: checkpoint between frames.  Import is refused with ASP_ERR_STATE when the record's
 * geometry or positions differ from the receiving batch's; advance that batch by the same calls first. */
size_t AspAudioBufferBatch_state_size(const AspAudioBufferBatch* b);
int AspAudioBufferBatch_ExportState(AspAudioBufferBatch* b, int stream, void* blob);
int AspAudioBufferBatch_ImportState(AspAudioBufferBatch* b, int stream, const void* blob);

#ifdef __cplusplus
}
#endif
#endif /* ASP_AUDIO_BUFFER_H_ */
