/* asp_bf.h -- batched WebRTC nonlinear beamformer on the GPU: webrtc::Beamformer
 * (modules/audio_processing/beamformer/ over common_audio's LappedTransform and Blocker) for num_streams
 * independent microphone arrays, bit-exact with the reference compiled in place (the FFT
 * seam is the reference's own WebRtc_rdft).  One batch has one uniform linear array geometry (2 to 8
 * microphones) shared by every stream; every stream has its own state.  The band rate is 16 kHz and a chunk is
 * 10 ms: 160 samples per microphone in, 160 samples of one channel out.  A 32 or 48 kHz stream passes its low
 * band here and, optionally, its next band as the high band (also 160 samples per chunk).
 *
 * Layouts (S streams, M microphones, F chunks):
 *   input           [F][S][M][160]
 *   high_input      [F][S][M][160]   or NULL: no high band in this call
 *   output          [F][S][160]
 *   high_output     [F][S][160]      or NULL (required with high_input)
 *   target_present  [F][S] uint8     or NULL: is_target_present() after each chunk
 * mem says where these arrays live: ASP_MEM_HOST or ASP_MEM_DEVICE (asp_ns.h), all in the same place.
 *
 * Return values: 0, or ASP_ERR_* (negative); AspNs_last_error() has the text.
 *
 * Unspecified in the reference, and here: a mask is NaN when a bin's delay-and-sum response is exactly zero
 * while its denominator passes the threshold; std::nth_element on such a row is unspecified. */
#ifndef ASP_BF_H_
#define ASP_BF_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASP_BF_MIN_MICS 2
#define ASP_BF_MAX_MICS 8
#define ASP_BF_CHUNK 160    /* samples per band and chunk */
#define ASP_BF_BINS 129     /* kFftSize / 2 + 1, kFftSize = 256 */
#define ASP_BF_BUFFER 384   /* the Blocker's buffers: chunk + initial delay (256 - gcd(160, 128) = 224) */

/* One stream's state.  The Blocker's buffers travel beside it as one float array: the input buffer [M][384],
 * then the output buffer [384]. */
typedef struct AspBfState {
  int32_t num_mics;
  int32_t frame_offset;                 /* Blocker::frame_offset_: cycles 0, 96, 64, 32 */
  int32_t current_block_ix, previous_block_ix;
  int32_t is_target_present, interference_blocks_count;
  float high_pass_postfilter_mask;      /* starts at 0 (the reference leaves it uninitialised) */
  int32_t reserved;
  float postfilter_masks[2][ASP_BF_BINS];
} AspBfState;

typedef struct AspBfBatch AspBfBatch;

size_t AspBf_state_size(void);

int AspBfBatch_Create(AspBfBatch** out, int num_streams, int device);
int AspBfBatch_Free(AspBfBatch* b);
int AspBfBatch_num_streams(const AspBfBatch* b);

/* The Beamformer constructor and Beamformer::Initialize for every stream.  geometry_xyz: [num_mics][3] metres.
 * ASP_ERR_PARAM, with the reason in AspNs_last_error(), for: num_mics outside 2..8; a geometry that is not a
 * uniform linear array where the reference CHECKs; chunk_size_ms other than 10; sample_rate_hz other than 16000
 * (at 8 kHz the reference's own bound high_frequency_upper_bin_bound_ <= kNumFreqBins does not hold; 32 and
 * 48 kHz streams come here band-split). */
int AspBfBatch_Initialize(AspBfBatch* b, int num_mics, const float* geometry_xyz, int chunk_size_ms,
                          int sample_rate_hz);
/* resets one stream of an initialised batch to its state after Initialize; the tables stay */
int AspBfBatch_InitializeStream(AspBfBatch* b, int stream);

/* Beamformer::ProcessChunk on one chunk of every stream */
int AspBfBatch_ProcessChunk(AspBfBatch* b, const float* input, const float* high_input, float* output,
                            float* high_output, uint8_t* target_present, int mem);
/* num_frames consecutive chunks in one launch: the state is read and written once */
int AspBfBatch_ProcessChunks(AspBfBatch* b, int num_frames, const float* input, const float* high_input,
                             float* output, float* high_output, uint8_t* target_present, int mem);

/* floats in a stream's buffer array: (M + 1) * 384; -1 before Initialize */
int AspBfBatch_state_floats(const AspBfBatch* b);
int AspBfBatch_GetState(AspBfBatch* b, int stream, AspBfState* state, float* buffers);
int AspBfBatch_SetState(AspBfBatch* b, int stream, const AspBfState* state, const float* buffers);

/* The Initialize-time tables, in the reference's element order.  which: 0 window_ [256], 1 wave_numbers_ [129],
 * 2 mask_thresholds_ [129], 3 delay_sum_masks_ [129][M][2], 4 target_cov_mats_ [129][M][M][2],
 * 5 interf_cov_mats_ [129][M][M][2] (the reflected ones are their conjugates), 6 rxiws_ [129], 7 rpsiws_ [129],
 * 8 reflected_rpsiws_ [129], 9 decay_threshold_ [1].  GetTables returns the number of floats written (cap: room
 * in floats), or ASP_ERR_PARAM.  SetTables replaces a table (count must be its length): for the tests, which
 * load the golden's tables so that the kernel's pin does not depend on the host's libm. */
int AspBfBatch_GetTables(AspBfBatch* b, int which, float* out, int cap);
int AspBfBatch_SetTables(AspBfBatch* b, int which, const float* in, int count);

int AspBfBatch_SetStream(AspBfBatch* b, void* hip_stream);
int AspBfBatch_Synchronize(AspBfBatch* b);

/* Test seam: out[i] = the kernel's hypotf (std::abs of a complex<float>) of (x[i], y[i]), evaluated on the
 * device.  x, y and out are host pointers to n floats. */
int AspBf_debug_hypotf(const float* x, const float* y, float* out, size_t n, int device);

#ifdef __cplusplus
}
#endif
#endif /* ASP_BF_H_ */
