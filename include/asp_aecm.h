/*
 * asp_aecm.h -- C-ABI of the MI355X batched mobile echo canceller: the reference's WebRtcAecm_*
 * (WebRtc_AMP_Port/webrtc/modules/audio_processing/aecm/: echo_control_mobile.c over aecm_core.c,
 * aecm_core_c.c, the fixed-point delay estimator and the spl FFT).  Integer arithmetic, bit-exact.
 *
 * Layer 1: the reference's entry points, signature-identical; each handle is a batch of one stream.
 * Layer 2: AspAecmBatch_*, N independent streams per call with every stream's state resident in HBM;
 * a call of F frames runs, for each frame and stream, "BufferFarend, then Process" in time order.
 * No CPU fallback: without a HIP device every Create fails.
 */
#ifndef ASP_AECM_H_
#define ASP_AECM_H_

#include <stddef.h>
#include <stdint.h>

#include "asp_ns.h" /* ASP_OK / ASP_ERR_*, ASP_MEM_HOST / ASP_MEM_DEVICE */

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- layer 1 */
enum { AecmFalse = 0, AecmTrue };

#define AECM_UNSPECIFIED_ERROR 12000
#define AECM_UNSUPPORTED_FUNCTION_ERROR 12001
#define AECM_UNINITIALIZED_ERROR 12002
#define AECM_NULL_POINTER_ERROR 12003
#define AECM_BAD_PARAMETER_ERROR 12004
#define AECM_BAD_PARAMETER_WARNING 12100

typedef struct {
  int16_t cngMode;  /* AecmFalse, AecmTrue (default) */
  int16_t echoMode; /* 0, 1, 2, 3 (default), 4 */
} AecmConfig;

int32_t WebRtcAecm_Create(void** aecmInst); /* -1 for NULL or when no HIP device is present */
int32_t WebRtcAecm_Free(void* aecmInst);
int32_t WebRtcAecm_Init(void* aecmInst, int32_t sampFreq); /* 8000 / 16000 */
int32_t WebRtcAecm_BufferFarend(void* aecmInst, const int16_t* farend, int16_t nrOfSamples);
int32_t WebRtcAecm_Process(void* aecmInst, const int16_t* nearendNoisy, const int16_t* nearendClean,
                           int16_t* out, int16_t nrOfSamples, int16_t msInSndCardBuf);
int32_t WebRtcAecm_set_config(void* aecmInst, AecmConfig config);
int32_t WebRtcAecm_get_config(void* aecmInst, AecmConfig* config);
int32_t WebRtcAecm_InitEchoPath(void* aecmInst, const void* echo_path, size_t size_bytes);
int32_t WebRtcAecm_GetEchoPath(void* aecmInst, void* echo_path, size_t size_bytes);
size_t WebRtcAecm_echo_path_size_bytes(void); /* 130 */
int32_t WebRtcAecm_get_error_code(void* aecmInst);

/* ---------------------------------------------------------------- layer 2 */
typedef struct AspAecmBatch AspAecmBatch;

typedef struct AspAecmRing { /* RingBuffer (ring_buffer.c) without its pointers */
  int32_t read_pos, write_pos, rw_wrap;
} AspAecmRing;

/* One stream's instance: AecMobile + AecmCore + the two fixed-point delay estimator structs, field by
 * field, with the ring buffers' storage inline and without pointers.  The delay estimator's float
 * histogram is left out: robust validation is disabled in AECM, so it stays zero. */
typedef struct AspAecmState {
  /* AecMobile (echo_control_mobile.c) */
  int32_t sampFreq, knownDelay, timeForDelayChange, ECstartup, checkBuffSize, delayChange;
  int16_t bufSizeStart, counter, sum, firstVal, checkBufSizeCtr, msInSndCardBuf, filtDelay, lastDelayDiff;
  int16_t echoMode, pad0;
  int16_t farendOld[2][80];
  AspAecmRing farendBuf;
  int16_t farendBuf_data[4000];
  /* AecmCore (aecm_core.h) */
  int32_t farBufWritePos, farBufReadPos, coreKnownDelay, lastKnownDelay, firstVAD;
  AspAecmRing farFrameBuf, nearNoisyFrameBuf, nearCleanFrameBuf, outFrameBuf;
  int16_t farFrameBuf_data[144], nearNoisyFrameBuf_data[144], nearCleanFrameBuf_data[144], outFrameBuf_data[144];
  int16_t farBuf[256];
  int16_t mult, pad1;
  uint32_t seed;
  /* DelayEstimatorFarend + BinaryDelayEstimatorFarend (history 100) */
  int32_t mean_far_spectrum[65], far_spectrum_initialized;
  uint32_t binary_far_history[100];
  int32_t far_bit_counts[100];
  /* DelayEstimator + BinaryDelayEstimator (lookahead 0) */
  int32_t mean_near_spectrum[65], near_spectrum_initialized;
  int32_t mean_bit_counts[101], bit_counts[100];
  uint32_t binary_near_history[1];
  int32_t minimum_probability, last_delay_probability, last_delay, last_candidate_delay, compare_delay,
      candidate_hits;
  /* far history */
  uint16_t far_history[65 * 100];
  int32_t far_history_pos, far_q_domains[100];
  int16_t nlpFlag, fixedDelay;
  uint32_t totCount;
  int16_t dfaCleanQDomain, dfaCleanQDomainOld, dfaNoisyQDomain, dfaNoisyQDomainOld;
  int16_t nearLogEnergy[64], farLogEnergy, echoAdaptLogEnergy[64], echoStoredLogEnergy[64];
  int16_t channelStored[65], channelAdapt16[65];
  int32_t channelAdapt32[65];
  int16_t xBuf[128], dBufClean[128], dBufNoisy[128], outBuf[64];
  int32_t echoFilt[65];
  int16_t nearFilt[65];
  int32_t noiseEst[65], noiseEstTooLowCtr[65], noiseEstTooHighCtr[65];
  int16_t noiseEstCtr, cngMode;
  int32_t mseAdaptOld, mseStoredOld, mseThreshold;
  int16_t farEnergyMin, farEnergyMax, farEnergyMaxMin, farEnergyVAD, farEnergyMSE;
  int32_t currentVADValue;
  int16_t vadUpdateCount, startupState, mseChannelCount, supGain, supGainOld, supGainErrParamA,
      supGainErrParamD, supGainErrParamDiffAB, supGainErrParamDiffBD;
} AspAecmState;

int AspAecmBatch_Create(AspAecmBatch** out, int num_streams, int device);
int AspAecmBatch_Free(AspAecmBatch* b);
int AspAecmBatch_num_streams(const AspAecmBatch* b);
int AspAecmBatch_Init(AspAecmBatch* b, int32_t sampFreq);               /* every stream */
int AspAecmBatch_InitStream(AspAecmBatch* b, int stream, int32_t sampFreq);
int AspAecmBatch_set_config(AspAecmBatch* b, AecmConfig config);         /* every stream */
int AspAecmBatch_set_config_stream(AspAecmBatch* b, int stream, AecmConfig config);
int AspAecmBatch_InitEchoPath_stream(AspAecmBatch* b, int stream, const int16_t* echo_path /* [65] */);
int AspAecmBatch_GetEchoPath_stream(AspAecmBatch* b, int stream, int16_t* echo_path /* [65] */);
/* far [num_streams][nrOfSamples] int16, every stream */
int AspAecmBatch_BufferFarend(AspAecmBatch* b, const int16_t* far, int nrOfSamples, int mem);
/* near / clean (nullable) / out [num_streams][nrOfSamples]; one msInSndCardBuf for all streams
 * (ProcessV: one per stream).  msInSndCardBuf outside [0, 500] is clamped and the stream's error code
 * set to AECM_BAD_PARAMETER_WARNING, as the reference does; the call then returns ASP_OK all the same
 * (per-stream return values: ProcessFrames). */
int AspAecmBatch_Process(AspAecmBatch* b, const int16_t* near, const int16_t* clean, int16_t* out,
                         int nrOfSamples, int16_t msInSndCardBuf, int mem);
int AspAecmBatch_ProcessV(AspAecmBatch* b, const int16_t* near, const int16_t* clean, int16_t* out,
                          int nrOfSamples, const int16_t* msInSndCardBuf /* [num_streams], host */, int mem);
/* F frames of "BufferFarend (far nullable: skipped), then Process": far / near / clean (nullable) / out
 * [F][num_streams][nrOfSamples], msInSndCardBuf [F][num_streams] (host).  ret (nullable, host,
 * [F][num_streams]) receives what WebRtcAecm_Process would have returned (0 or -1).  mem: ASP_MEM_*; for
 * ASP_MEM_DEVICE the audio buffers live on the device (ordered on the batch's stream), for ASP_MEM_HOST
 * they are copied in / out; either way the call returns when the frames are done. */
int AspAecmBatch_ProcessFrames(AspAecmBatch* b, int num_frames, const int16_t* far, const int16_t* near,
                               const int16_t* clean, int16_t* out, int nrOfSamples,
                               const int16_t* msInSndCardBuf, int32_t* ret, int mem);
int AspAecmBatch_get_error_code(AspAecmBatch* b, int stream);
int AspAecmBatch_ExportState(AspAecmBatch* b, int stream, AspAecmState* out);
int AspAecmBatch_ImportState(AspAecmBatch* b, int stream, const AspAecmState* in);
int AspAecmBatch_SetStream(AspAecmBatch* b, void* hip_stream); /* NULL: back to the batch's own stream */
int AspAecmBatch_Synchronize(AspAecmBatch* b);
size_t AspAecm_state_size(void); /* sizeof(AspAecmState) */

#ifdef __cplusplus
}
#endif
#endif /* ASP_AECM_H_ */
