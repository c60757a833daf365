/* asp_hpf.h -- batched WebRTC high-pass filter on the GPU: HighPassFilterImpl's fixed-point biquad
 * (modules/audio_processing/high_pass_filter_impl.cc) for num_streams independent streams of num_channels
 * channels each, bit-exact with the reference built for x86-64.  Every stream-channel has
 * its own AspHpfState; streams of one batch may differ in coefficient set (AspHpfBatch_InitStream).
 *
 * Layout (S streams, C channels, n samples, F frames): in and out are [F][S][C][n], n the length of band 0 of a
 * 10 ms frame (80 at 8 kHz, 160 at every other rate; any 1 <= n <= ASP_HPF_MAX_SAMPLES is served).  in == out is
 * allowed; otherwise the two must not overlap.  mem says where the arrays live: ASP_MEM_HOST (copied in and out,
 * the call returns when done) or ASP_MEM_DEVICE (the call returns once the launch is queued on the batch's HIP
 * stream; AspHpfBatch_Synchronize waits).
 *
 * Return values: 0, or ASP_ERR_* (asp_ns.h); AspNs_last_error() has the text.  There is no CPU path. */
#ifndef ASP_HPF_H_
#define ASP_HPF_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASP_HPF_MAX_SAMPLES 160

/* FilterState: y holds the last two outputs split into high and low parts (y[0], y[1] the newest), x the last
 * two inputs; coeff_set 0 is kFilterCoefficients8kHz, 1 kFilterCoefficients. */
typedef struct AspHpfState {
  int16_t y[4];
  int16_t x[2];
  int16_t coeff_set;
  int16_t reserved;
} AspHpfState;

typedef struct AspHpfBatch AspHpfBatch;

size_t AspHpf_state_size(void);

int AspHpfBatch_Create(AspHpfBatch** out, int num_streams, int num_channels, int device);
int AspHpfBatch_Free(AspHpfBatch* b);
int AspHpfBatch_num_streams(const AspHpfBatch* b);
int AspHpfBatch_num_channels(const AspHpfBatch* b);

/* InitializeFilter for every channel of every stream, or of one stream: sample_rate_hz 8000 picks the 8 kHz
 * coefficients, 16000 / 32000 / 48000 the others; any other rate is ASP_ERR_PARAM. */
int AspHpfBatch_Init(AspHpfBatch* b, int sample_rate_hz);
int AspHpfBatch_InitStream(AspHpfBatch* b, int stream, int sample_rate_hz);

/* Filter on num_frames consecutive frames; the state is read and written once.  ASP_ERR_STATE before Init. */
int AspHpfBatch_Process(AspHpfBatch* b, const int16_t* in, int16_t* out, int num_frames, int samples, int mem);
/* The same on FloatS16 samples: FloatS16ToS16, the filter, back to float (the int16 view of a float buffer). */
int AspHpfBatch_ProcessFloatS16(AspHpfBatch* b, const float* in, float* out, int num_frames, int samples, int mem);

int AspHpfBatch_ExportState(AspHpfBatch* b, int stream, int channel, AspHpfState* state);
int AspHpfBatch_ImportState(AspHpfBatch* b, int stream, int channel, const AspHpfState* state);

int AspHpfBatch_SetStream(AspHpfBatch* b, void* hip_stream);
int AspHpfBatch_Synchronize(AspHpfBatch* b);

/* Layer 1: one filter (a batch of one stream and one channel on device 0), host buffers, in place. */
typedef struct AspHpf AspHpf;
int AspHpf_Create(AspHpf** out);
int AspHpf_Init(AspHpf* h, int sample_rate_hz);
int AspHpf_Process(AspHpf* h, int16_t* data, int length);
int AspHpf_Free(AspHpf* h);

#ifdef __cplusplus
}
#endif
#endif /* ASP_HPF_H_ */
