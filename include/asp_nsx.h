/*
 * asp_nsx.h -- C-ABI of the MI355X batched fixed-point noise suppressor: the reference's WebRtcNsx_*
 * (WebRtc_AMP_Port/webrtc/modules/audio_processing/ns/: noise_suppression_x.c over nsx_core.c,
 * nsx_core_c.c and the spl FFT).  Integer arithmetic, bit-exact.
 *
 * Layer 1: the reference's entry points, signature-identical; each handle is a batch of one stream.
 * Layer 2: AspNsxBatch_*, N independent streams per call with every stream's state resident in HBM.
 * No CPU fallback: without a HIP device every Create fails.
 */
#ifndef ASP_NSX_H_
#define ASP_NSX_H_
#include <stddef.h>
#include <stdint.h>
#include "asp_ns.h" /* ASP_OK / ASP_ERR_*, ASP_MEM_HOST / ASP_MEM_DEVICE */
#ifdef __cplusplus
extern "C" {
#endif
/* ---------------------------------------------------------------- layer 1 */
typedef struct NsxHandleT NsxHandle;
int WebRtcNsx_Create(NsxHandle** nsxInst); /* -1 for NULL or when no HIP device is present */
int WebRtcNsx_Free(NsxHandle* nsxInst);
int WebRtcNsx_Init(NsxHandle* nsxInst, uint32_t fs);   /* 8000 / 16000 / 32000 / 48000, else -1 */
int WebRtcNsx_set_policy(NsxHandle* nsxInst, int mode); /* 0..3, else -1 */
/* speechFrame / outFrame: num_bands pointers to 80 (8 kHz) or 160 samples; outFrame[i] == speechFrame[i]
 * is allowed.  The reference returns void and asserts on a handle that was not initialised and on more
 * than three bands; here such a call (and a NULL argument or num_bands < 1) prints a line on stderr,
 * leaves outFrame and the state untouched, and AspNsx_last_refused() returns 1 until the next good call. */
void WebRtcNsx_Process(NsxHandle* nsxInst, const short* const* speechFrame, int num_bands,
                       short* const* outFrame);
int AspNsx_last_refused(void); /* per thread */
/* ---------------------------------------------------------------- layer 2 */
typedef struct AspNsxBatch AspNsxBatch;
/* One stream's instance: NoiseSuppressionFixedC field by field, in its order, without its three
 * pointers (window, factor2Table, real_fft: they follow from fs and aggrMode). */
typedef struct AspNsxState {
  uint32_t fs;
  int16_t analysisBuffer[256], synthesisBuffer[256];
  uint16_t noiseSupFilter[129], overdrive, denoiseBound;
  int16_t noiseEstLogQuantile[3 * 129], noiseEstDensity[3 * 129], noiseEstCounter[3], noiseEstQuantile[129];
  int32_t anaLen, anaLen2, magnLen, aggrMode, stages, initFlag, gainMap;
  int32_t maxLrt, minLrt, logLrtTimeAvgW32[129], featureLogLrt, thresholdLogLrt;
  int16_t weightLogLrt;
  uint32_t featureSpecDiff, thresholdSpecDiff;
  int16_t weightSpecDiff;
  uint32_t featureSpecFlat, thresholdSpecFlat;
  int16_t weightSpecFlat;
  int32_t avgMagnPause[129];
  uint32_t magnEnergy, sumMagn, curAvgMagnEnergy, timeAvgMagnEnergy, timeAvgMagnEnergyTmp, whiteNoiseLevel;
  uint32_t initMagnEst[129];
  int32_t pinkNoiseNumerator, pinkNoiseExp, minNorm, zeroInputSignal;
  uint32_t prevNoiseU32[129];
  uint16_t prevMagnU16[129];
  int16_t priorNonSpeechProb;
  int32_t blockIndex, modelUpdate, cntThresUpdate;
  int16_t histLrt[1000], histSpecFlat[1000], histSpecDiff[1000];
  int16_t dataBufHBFX[2][256];
  int32_t qNoise, prevQNoise, prevQMagn, blockLen10ms;
  int16_t real[256], imag[256];
  int32_t energyIn, scaleEnergyIn, normData;
} AspNsxState;
int AspNsxBatch_Create(AspNsxBatch** out, int num_streams, int device);
int AspNsxBatch_Free(AspNsxBatch* b);
int AspNsxBatch_num_streams(const AspNsxBatch* b);
int AspNsxBatch_Init(AspNsxBatch* b, uint32_t fs);                    /* every stream; policy back to 0 */
int AspNsxBatch_InitStream(AspNsxBatch* b, int stream, uint32_t fs);
int AspNsxBatch_set_policy(AspNsxBatch* b, int mode);                 /* every stream */
int AspNsxBatch_set_policy_stream(AspNsxBatch* b, int stream, int mode);
/* Streams of one batch may differ in mode and in where they are in their run (per-stream InitStream at
 * any time).  One frame length per call: samples_per_band is 80 or 160, and a call in which any stream was
 * initialised for the other length (8000 against the rest), or not at all, is refused with ASP_ERR_STATE
 * before anything runs.
 * low_in / low_out [num_frames][num_streams][n]; high_in / high_out [num_frames][num_bands - 1][num_streams][n]
 * (NULL for one band); in-place allowed.  mem: ASP_MEM_*; ASP_MEM_HOST copies in / out; either way the
 * call returns when the frames are done. */
int AspNsxBatch_Process(AspNsxBatch* b, const int16_t* low_in, const int16_t* high_in, int16_t* low_out,
                        int16_t* high_out, int num_bands, int samples_per_band, int mem);
int AspNsxBatch_ProcessFrames(AspNsxBatch* b, int num_frames, const int16_t* low_in, const int16_t* high_in,
                              int16_t* low_out, int16_t* high_out, int num_bands, int samples_per_band, int mem);
int AspNsxBatch_ExportState(AspNsxBatch* b, int stream, AspNsxState* out);
int AspNsxBatch_ImportState(AspNsxBatch* b, int stream, const AspNsxState* in);
int AspNsxBatch_SetStream(AspNsxBatch* b, void* hip_stream); /* NULL: back to the batch's own stream */
int AspNsxBatch_Synchronize(AspNsxBatch* b);
size_t AspNsx_state_size(void); /* sizeof(AspNsxState) */
#ifdef __cplusplus
}
#endif
#endif /* ASP_NSX_H_ */
