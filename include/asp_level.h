/* asp_level.h -- batched WebRTC level estimator on the GPU: LevelEstimatorImpl over RMSLevel
 * (modules/audio_processing/level_estimator_impl.cc, rms_level.cc) for num_streams independent streams, bit-exact
 * with the reference built for x86-64: the float sum of squares is accumulated one sample
 * at a time, channel 0's samples of a frame first, then channel 1's, as the reference does.
 *
 * Layout (S streams, C channels, n samples, F frames): in is [F][S][C][n], n <= ASP_LEVEL_MAX_SAMPLES, in host or
 * device memory (mem: ASP_MEM_HOST / ASP_MEM_DEVICE, asp_ns.h; a device call returns once its launch is queued
 * on the batch's HIP stream).  A new batch is reset.
 *
 * Return values: 0, or ASP_ERR_* (asp_ns.h); AspNs_last_error() has the text.  There is no CPU path. */
#ifndef ASP_LEVEL_H_
#define ASP_LEVEL_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASP_LEVEL_MAX_SAMPLES 480
#define ASP_LEVEL_MAX_CHANNELS 16
#define ASP_LEVEL_MIN 127 /* RMSLevel::kMinLevel */

/* RMSLevel's members */
typedef struct AspLevelState {
  float sum_square;
  int32_t sample_count;
} AspLevelState;

typedef struct AspLevelBatch AspLevelBatch;

size_t AspLevel_state_size(void);

int AspLevelBatch_Create(AspLevelBatch** out, int num_streams, int device);
int AspLevelBatch_Free(AspLevelBatch* b);
int AspLevelBatch_num_streams(const AspLevelBatch* b);

int AspLevelBatch_Reset(AspLevelBatch* b);
int AspLevelBatch_ResetStream(AspLevelBatch* b, int stream);

/* RMSLevel::Process on every channel of num_frames consecutive frames */
int AspLevelBatch_Process(AspLevelBatch* b, const int16_t* in, int num_frames, int num_channels, int samples, int mem);
/* RMSLevel::ProcessMuted(length) on every stream, or on one */
int AspLevelBatch_ProcessMuted(AspLevelBatch* b, int length);
int AspLevelBatch_ProcessMutedStream(AspLevelBatch* b, int stream, int length);

/* RMSLevel::RMS(): waits for the batch's work, evaluates the reference's expression on the host (out: host memory,
 * [num_streams], or one value), and resets what it read: 0 (full scale) .. 127 (ASP_LEVEL_MIN, also for silence). */
int AspLevelBatch_RMS(AspLevelBatch* b, int32_t* out);
int AspLevelBatch_RMS_stream(AspLevelBatch* b, int stream, int32_t* out);

int AspLevelBatch_ExportState(AspLevelBatch* b, int stream, AspLevelState* state);
int AspLevelBatch_ImportState(AspLevelBatch* b, int stream, const AspLevelState* state);

int AspLevelBatch_SetStream(AspLevelBatch* b, void* hip_stream);
int AspLevelBatch_Synchronize(AspLevelBatch* b);

#ifdef __cplusplus
}
#endif
#endif /* ASP_LEVEL_H_ */
