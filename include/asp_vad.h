/*
 * asp_vad.h -- C-ABI of the MI355X batched voice activity detector: the reference's WebRtcVad_*
 * (WebRtc_AMP_Port/webrtc/common_audio/vad/webrtc_vad.c:24-129 over vad_core.c, vad_filterbank.c,
 * vad_gmm.c, vad_sp.c and the 48 -> 8 kHz spl resampler).  Integer arithmetic, bit-exact.
 *
 * Layer 1: the reference's entry points, signature-identical; each handle is a batch of one stream.
 * Layer 2: AspVadBatch_*, N independent streams per call with every stream's VadInstT resident in HBM;
 * a call of F frames loads each stream's state once, runs the frames in time order on chip and stores
 * it once.  No CPU fallback: without a HIP device every Create fails.
 */
#ifndef ASP_VAD_H_
#define ASP_VAD_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h" /* ASP_OK / ASP_ERR_*, ASP_MEM_HOST / ASP_MEM_DEVICE */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- layer 1 */
typedef struct WebRtcVadInst VadInst;

int WebRtcVad_Create(VadInst** handle);   /* -1 for NULL or when no HIP device is present */
void WebRtcVad_Free(VadInst* handle);
int WebRtcVad_Init(VadInst* handle);      /* WebRtcVad_InitCore; mode 0 */
int WebRtcVad_set_mode(VadInst* handle, int mode);  /* 0..3; -1 when not initialised */
/* 1 speech, 0 no speech, -1 on a NULL / uninitialised handle, NULL frame, invalid rate or length */
int WebRtcVad_Process(VadInst* handle, int fs, const int16_t* audio_frame, int frame_length);
int WebRtcVad_ValidRateAndFrameLength(int rate, int frame_length);

/* ---------------------------------------------------------------- layer 2 */
typedef struct AspVadBatch AspVadBatch;

/* One stream's instance: VadInstT (vad_core.h:27-57) field by field, same layout (736 bytes);
 * S_* are WebRtcSpl_State48khzTo8khz (signal_processing_library.h:890-896). */
typedef struct AspVadState {
  int32_t vad;
  int32_t downsampling_filter_states[4];
  int32_t S_48_24[8];
  int32_t S_24_24[16];
  int32_t S_24_16[8];
  int32_t S_16_8[8];
  int16_t noise_means[12];
  int16_t speech_means[12];
  int16_t noise_stds[12];
  int16_t speech_stds[12];
  int32_t frame_counter;
  int16_t over_hang;
  int16_t num_of_speech;
  int16_t index_vector[96];
  int16_t low_value_vector[96];
  int16_t mean_value[6];
  int16_t upper_state[5];
  int16_t lower_state[5];
  int16_t hp_filter_state[4];
  int16_t over_hang_max_1[3];
  int16_t over_hang_max_2[3];
  int16_t individual[3];
  int16_t total[3];
  int32_t init_flag;
} AspVadState;

int AspVadBatch_Create(AspVadBatch** out, int num_streams, int device);
int AspVadBatch_Free(AspVadBatch* b);
int AspVadBatch_num_streams(const AspVadBatch* b);
int AspVadBatch_Init(AspVadBatch* b);                     /* WebRtcVad_InitCore for every stream */
int AspVadBatch_set_mode(AspVadBatch* b, int mode);       /* every stream; ASP_ERR_STATE before Init */
/* one stream; the others are untouched; ordered on the batch's HIP stream */
int AspVadBatch_InitStream(AspVadBatch* b, int stream);
int AspVadBatch_set_mode_stream(AspVadBatch* b, int stream, int mode);
/* in [num_frames][num_streams][frame_length] int16 -> decisions [num_frames][num_streams] (0 / 1, what
 * WebRtcVad_Process returns), levels [num_frames][num_streams] (nullable: the raw CalcVad* value, the
 * hangover-weighted vadflag).  fs and frame_length are per call, as in the reference.  mem: ASP_MEM_*;
 * for ASP_MEM_DEVICE the call is asynchronous on the batch's stream and the buffers must be 4-byte
 * aligned; ASP_MEM_HOST copies in / out and returns when done. */
int AspVadBatch_Process(AspVadBatch* b, int fs, int frame_length, const int16_t* in, int num_frames,
                        int8_t* decisions, int32_t* levels, int mem);
int AspVadBatch_ExportState(AspVadBatch* b, int stream, AspVadState* out);
int AspVadBatch_ImportState(AspVadBatch* b, int stream, const AspVadState* in);
int AspVadBatch_SetStream(AspVadBatch* b, void* hip_stream);  /* NULL: back to the batch's own stream */
int AspVadBatch_Synchronize(AspVadBatch* b);

/* ---- test seams ----
 * WebRtcVad_CalculateFeatures (vad_filterbank.c:247-334) for every stream: in [num_streams][frame_length]
 * int16 at 8 kHz (80 / 160 / 240) -> features [num_streams][7] int16 (six log energies, then the total
 * energy); the filter states of each stream advance as in the reference. */
int AspVadBatch_Features(AspVadBatch* b, const int16_t* in, int frame_length, int16_t* features, int mem);
/* WebRtcVad_GaussianProbability (vad_gmm.c:30-83) on the device over n (input, mean, std) triples, host
 * arrays: probability [n] int32, delta [n] int16. */
int AspVad_debug_gaussian(const int16_t* input, const int16_t* mean, const int16_t* std_, int n,
                          int32_t* probability, int16_t* delta, int device);

#ifdef __cplusplus
}
#endif
#endif /* ASP_VAD_H_ */
