/* asp_ts.h -- batched WebRTC transient (keyclick) suppressor on the GPU: webrtc::TransientSuppressor
 * (modules/audio_processing/transient/) for num_streams independent streams, bit-exact with the reference
 * built for x86-64.  One batch has one sample rate, one detection rate and one channel
 * count; every stream has its own state.  A chunk is 10 ms.
 *
 * Layouts (S streams, C channels, L = sample_rate / 100, D = detection_rate / 100, F chunks):
 *   data               [F][S][C][L]   in place: the delayed (and, once enabled, suppressed) audio comes back
 *   detection_data     [F][S][D]      or NULL: the newest chunk of the first channel is used (D must be <= L)
 *   reference_data     [F][S][R]      or NULL: no stream has a reference in this call
 *   reference_present  [F][S]         or NULL: every stream has one (only read when reference_data is given)
 *   voice_probability  [F][S]
 *   key_pressed        [F][S]
 *   results            [F][S]         or NULL: 0, or -1 where the reference's Suppress returns -1 for that stream
 *                                     (a voice probability outside [0, 1]); such a chunk leaves the stream's
 *                                     state and its data untouched
 * mem says where these arrays live: ASP_MEM_HOST or ASP_MEM_DEVICE (asp_ns.h), all in the same place.
 *
 * Return values: the reference's 0 / -1 where it has one (-1 from Suppress* also when any stream's result is
 * -1), ASP_ERR_* (negative, below -1) for this library's own failures; AspNs_last_error() has the text. */
#ifndef ASP_TS_H_
#define ASP_TS_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASP_TS_LEAVES 8      /* leaves of the 3-level wavelet packet tree */
#define ASP_TS_NODES 7       /* nodes that have children: the root, 2 and 4 */
#define ASP_TS_HISTORY 15    /* FIR history of a node's children: 16 taps */
#define ASP_TS_MAX_QUEUE 180 /* moving-moment queue at 48 kHz (30 ms of leaf samples) */

/* One stream's scalar and detector state.  The three large buffers (in_buffer_, out_buffer_, spectral_mean_)
 * travel beside it as one float array: in [C][N], out [C][N], mean [C][N / 2 + 1], N the analysis length. */
typedef struct AspTsState {
  int32_t sample_rate_hz, detection_rate_hz, num_channels;
  float detector_smoothed;
  int32_t keypress_counter, chunks_since_keypress;
  int32_t detection_enabled, suppression_enabled, use_hard_restoration;
  int32_t chunks_since_voice_change;
  uint32_t seed;
  int32_t using_reference;
  /* TransientDetector */
  int32_t chunks_at_startup_left_to_delete;
  float reference_energy;
  int32_t detector_using_reference;
  float previous_results[3];                  /* oldest first */
  float last_first_moment[ASP_TS_LEAVES], last_second_moment[ASP_TS_LEAVES];
  /* MovingMoments of the leaves; the queue is a ring of three chunks, queue_pos (0..2) the oldest third */
  float moment_sum[ASP_TS_LEAVES], moment_sum_of_squares[ASP_TS_LEAVES];
  int32_t queue_pos;
  float moment_queue[ASP_TS_LEAVES][ASP_TS_MAX_QUEUE];
  /* the last 15 samples of the root (0), the level-1 nodes (1, 2) and the level-2 nodes (3..6): the filter
   * state of both children of that node */
  float node_history[ASP_TS_NODES][ASP_TS_HISTORY];
} AspTsState;

typedef struct AspTsBatch AspTsBatch;

size_t AspTs_state_size(void);

int AspTsBatch_Create(AspTsBatch** out, int num_streams, int device);
int AspTsBatch_Free(AspTsBatch* b);
int AspTsBatch_num_streams(const AspTsBatch* b);

/* TransientSuppressor::Initialize for every stream; -1 where the reference returns -1 */
int AspTsBatch_Initialize(AspTsBatch* b, int sample_rate_hz, int detection_rate_hz, int num_channels);
/* the same for one stream of an initialised batch (the batch's rates and channel count) */
int AspTsBatch_InitializeStream(AspTsBatch* b, int stream);

/* floats in a stream's buffer array: C * (2 N + N / 2 + 1); -1 before Initialize */
int AspTsBatch_state_floats(const AspTsBatch* b);
int AspTsBatch_GetState(AspTsBatch* b, int stream, AspTsState* state, float* buffers);
int AspTsBatch_SetState(AspTsBatch* b, int stream, const AspTsState* state, const float* buffers);

/* TransientSuppressor::Suppress on one chunk of every stream */
int AspTsBatch_Suppress(AspTsBatch* b, float* data, size_t data_length, int num_channels, const float* detection_data,
                        size_t detection_length, const float* reference_data, size_t reference_length,
                        const uint8_t* reference_present, const float* voice_probability, const uint8_t* key_pressed,
                        int32_t* results, int mem);
/* num_frames consecutive chunks in one launch: the state is read and written once */
int AspTsBatch_SuppressFrames(AspTsBatch* b, int num_frames, float* data, size_t data_length, int num_channels,
                              const float* detection_data, size_t detection_length, const float* reference_data,
                              size_t reference_length, const uint8_t* reference_present,
                              const float* voice_probability, const uint8_t* key_pressed, int32_t* results, int mem);

/* the Create-time tables, for the tests: which = 0 window, 1 FFT w (n / 2 floats: makewt then makect),
 * 2 mean_factor_ (n / 2 + 1); n = 128, 256, 512 or 1024.  Returns the number of floats written, or ASP_ERR_PARAM. */
int AspTs_table(int which, int n, float* out, int cap);

int AspTsBatch_SetStream(AspTsBatch* b, void* hip_stream);
int AspTsBatch_Synchronize(AspTsBatch* b);

#ifdef __cplusplus
}
#endif
#endif /* ASP_TS_H_ */
