/*
 * asp_agc.h -- C-ABI of the MI355X batched legacy gain control: the reference's WebRtcAgc_*
 * (WebRtc_AMP_Port/webrtc/modules/audio_processing/agc/legacy/: analog_agc.c over digital_agc.c and the
 * spl primitives they use).  Integer arithmetic, bit-exact.
 *
 * Layer 1: the reference's entry points (gain_control.h), signature-identical; each handle is a batch of
 *          one stream.
 * Layer 2: AspAgcBatch_*, N independent streams per call with every stream's state resident in HBM.
 * No CPU fallback: without a HIP device every Create fails.
 *
 * Where layer 1 differs from the reference (the reference would crash or read garbage; here the call
 * returns -1 and the state is untouched):
 *   - a NULL handle or a NULL pointer argument (band pointers included) in any entry point;
 *   - AddFarend / AddMic / VirtualMic / Process before a successful Init (set_config / get_config before
 *     Init return -1 with AGC_UNINITIALIZED_ERROR as lastError would have it, as in the reference);
 *   - num_bands outside 1..3;
 *   - Init with fs outside 8000 / 16000 / 32000 / 48000 (the reference only notices at Process), and Init
 *     with a mode outside 0..3 (the reference returns -1 after half an Init; here nothing is written);
 *   - fields that WebRtcAgc_Init leaves as malloc gave them (Rxx16w32_array[1], lowLevelSignal before the
 *     last line of Init, ...) are zero after Create.
 * Init with minLevel >= maxLevel or maxLevel above 2^26 - 1 returns -1 after initialising, as the
 * reference does.
 */
#ifndef ASP_AGC_H_
#define ASP_AGC_H_
#include <stddef.h>
#include <stdint.h>
#include "asp_ns.h" /* ASP_OK / ASP_ERR_*, ASP_MEM_HOST / ASP_MEM_DEVICE */
#ifdef __cplusplus
extern "C" {
#endif
/* ---------------------------------------------------------------- layer 1 (gain_control.h) */
/* a translation unit that has the reference's gain_control.h already keeps that header's declarations */
#ifndef WEBRTC_MODULES_AUDIO_PROCESSING_AGC_LEGACY_GAIN_CONTROL_H_
#define AGC_UNSPECIFIED_ERROR 18000
#define AGC_UNSUPPORTED_FUNCTION_ERROR 18001
#define AGC_UNINITIALIZED_ERROR 18002
#define AGC_NULL_POINTER_ERROR 18003
#define AGC_BAD_PARAMETER_ERROR 18004
#define AGC_BAD_PARAMETER_WARNING 18050
enum { kAgcModeUnchanged, kAgcModeAdaptiveAnalog, kAgcModeAdaptiveDigital, kAgcModeFixedDigital };
enum { kAgcFalse = 0, kAgcTrue };
typedef struct {
  int16_t targetLevelDbfs;   /* default 3 (-3 dBOv) */
  int16_t compressionGaindB; /* default 9 dB */
  uint8_t limiterEnable;     /* default kAgcTrue */
} WebRtcAgcConfig;
int WebRtcAgc_Create(void** agcInst); /* -1 for NULL or when no HIP device is present */
int WebRtcAgc_Free(void* agcInst);
int WebRtcAgc_Init(void* agcInst, int32_t minLevel, int32_t maxLevel, int16_t agcMode, uint32_t fs);
int WebRtcAgc_set_config(void* agcInst, WebRtcAgcConfig config);
int WebRtcAgc_get_config(void* agcInst, WebRtcAgcConfig* config);
/* samples: 80 at 8 kHz, 160 at 16 / 32 / 48 kHz, else -1 */
int WebRtcAgc_AddFarend(void* agcInst, const int16_t* inFar, int16_t samples);
int WebRtcAgc_AddMic(void* agcInst, int16_t* const* inMic, int16_t num_bands, int16_t samples);
int WebRtcAgc_VirtualMic(void* agcInst, int16_t* const* inMic, int16_t num_bands, int16_t samples,
                         int32_t micLevelIn, int32_t* micLevelOut);
int WebRtcAgc_Process(void* agcInst, const int16_t* const* inNear, int16_t num_bands, int16_t samples,
                      int16_t* const* out, int32_t inMicLevel, int32_t* outMicLevel, int16_t echo,
                      uint8_t* saturationWarning);
#endif
/* ---------------------------------------------------------------- layer 2 */
typedef struct AspAgcBatch AspAgcBatch;
/* One stream's instance: LegacyAgc field by field, in its order; AgcVad (vadMic, vadNearend, vadFarend)
 * and DigitalAgc flattened; without the debug FILE*s and the MIC_LEVEL_FEEDBACK fields.  Every field that
 * WebRtcAgc_Init does not write is zero after Create. */
#define ASP_AGC_VAD_FIELDS(p)                                                                     \
  int32_t p##_downState[8];                                                                       \
  int16_t p##_HPstate, p##_counter, p##_logRatio, p##_meanLongTerm;                               \
  int32_t p##_varianceLongTerm;                                                                   \
  int16_t p##_stdLongTerm, p##_meanShortTerm;                                                     \
  int32_t p##_varianceShortTerm;                                                                  \
  int16_t p##_stdShortTerm;
typedef struct AspAgcState {
  uint32_t fs;
  int16_t compressionGaindB, targetLevelDbfs, agcMode;
  uint8_t limiterEnable;
  int16_t defaultConfig_targetLevelDbfs, defaultConfig_compressionGaindB;
  uint8_t defaultConfig_limiterEnable;
  int16_t usedConfig_targetLevelDbfs, usedConfig_compressionGaindB;
  uint8_t usedConfig_limiterEnable;
  int16_t initFlag, lastError;
  int32_t analogTargetLevel, startUpperLimit, startLowerLimit, upperPrimaryLimit, lowerPrimaryLimit;
  int32_t upperSecondaryLimit, lowerSecondaryLimit;
  uint16_t targetIdx;
  int16_t analogTarget;
  int32_t filterState[8], upperLimit, lowerLimit, Rxx160w32, Rxx16_LPw32, Rxx160_LPw32, Rxx16_LPw32Max;
  int32_t Rxx16_vectorw32[10], Rxx16w32_array[2][5], env[2][10];
  int16_t Rxx16pos, envSum, vadThreshold, inActive, msTooLow, msTooHigh, changeToSlowMode, firstCall, msZero;
  int16_t msecSpeechOuterChange, msecSpeechInnerChange, activeSpeech, muteGuardMs, inQueue;
  int32_t micRef;
  uint16_t gainTableIdx;
  int32_t micGainIdx, micVol, maxLevel, maxAnalog, maxInit, minLevel, minOutput, zeroCtrlMax, lastInMicLevel;
  int16_t scale;
  ASP_AGC_VAD_FIELDS(vadMic)
  int32_t digitalAgc_capacitorSlow, digitalAgc_capacitorFast, digitalAgc_gain, digitalAgc_gainTable[32];
  int16_t digitalAgc_gatePrevious, digitalAgc_agcMode;
  ASP_AGC_VAD_FIELDS(vadNearend)
  ASP_AGC_VAD_FIELDS(vadFarend)
  int16_t lowLevelSignal;
} AspAgcState;
size_t AspAgc_state_size(void); /* sizeof(AspAgcState) */
/* CalculateGainTable on the host (what set_config runs): 32 Q16 gains; -1 as the reference returns it */
int AspAgc_gain_table(int32_t* table, int16_t compressionGaindB, int16_t targetLevelDbfs, uint8_t limiterEnable,
                      int16_t analogTarget);

int AspAgcBatch_Create(AspAgcBatch** out, int num_streams, int device);
int AspAgcBatch_Free(AspAgcBatch* b);
int AspAgcBatch_num_streams(const AspAgcBatch* b);
/* WebRtcAgc_Init on every stream / one stream.  Returns the reference's return value (0 / -1), or ASP_ERR_*.
 * The stream's stored mic level (below) becomes its micVol after Init: maxLevel, or 127 in adaptive-digital. */
int AspAgcBatch_Init(AspAgcBatch* b, int32_t min_level, int32_t max_level, int16_t mode, uint32_t fs);
int AspAgcBatch_InitStream(AspAgcBatch* b, int stream, int32_t min_level, int32_t max_level, int16_t mode, uint32_t fs);
/* WebRtcAgc_set_config; the gain table is recomputed on the host with the code the kernel would run.
 * 0 / -1 as the reference; last_error_stream gives the stream's lastError. */
int AspAgcBatch_set_config(AspAgcBatch* b, WebRtcAgcConfig config);
int AspAgcBatch_set_config_stream(AspAgcBatch* b, int stream, WebRtcAgcConfig config);
int AspAgcBatch_get_config_stream(AspAgcBatch* b, int stream, WebRtcAgcConfig* config);
int AspAgcBatch_last_error_stream(AspAgcBatch* b, int stream);
/* The level a stream hands to the next ProcessFrames call that passes mic_level_in == NULL. */
int AspAgcBatch_set_mic_level(AspAgcBatch* b, int32_t level);
int AspAgcBatch_set_mic_level_stream(AspAgcBatch* b, int stream, int32_t level);
int AspAgcBatch_get_mic_level_stream(AspAgcBatch* b, int stream, int32_t* level);
/* Streams of one batch may differ in mode, config and in where they are in their run.  One frame length per
 * call: samples_per_band is 80 or 160, and a call in which any stream was initialised for the other length,
 * or not at all, is refused with ASP_ERR_STATE before anything runs.
 * Audio: low [num_frames][num_streams][n]; high [num_frames][num_bands - 1][num_streams][n] (NULL for one
 * band); far [num_frames][num_streams][n].  Per-stream scalars: [num_frames][num_streams].  mem: ASP_MEM_*,
 * for every pointer of the call alike; ASP_MEM_HOST copies in / out; either way the call returns when the
 * frames are done.  The reference's per-stream return values of the call (0 / -1; for ProcessFrames the
 * frame's Process value) are kept [num_frames][num_streams] until the next call: AspAgcBatch_returns. */
int AspAgcBatch_AddFarend(AspAgcBatch* b, const int16_t* far, int samples, int mem);
int AspAgcBatch_AddMic(AspAgcBatch* b, int16_t* low, int16_t* high, int num_bands, int samples_per_band, int mem);
int AspAgcBatch_VirtualMic(AspAgcBatch* b, int16_t* low, int16_t* high, int num_bands, int samples_per_band,
                           const int32_t* mic_level_in, int32_t* mic_level_out, int mem);
/* echo NULL: 0; in-place allowed */
int AspAgcBatch_Process(AspAgcBatch* b, const int16_t* low_in, const int16_t* high_in, int16_t* low_out,
                        int16_t* high_out, int num_bands, int samples_per_band, const int32_t* mic_level_in,
                        const int16_t* echo, int32_t* mic_level_out, uint8_t* saturation, int mem);
/* The fused call, one launch for num_frames frames: per stream and frame AddFarend (far != NULL), then AddMic
 * (adaptive-analog streams) or VirtualMic (adaptive-digital streams) or neither, then Process on what that
 * left.  low_in / high_in are not written; in-place allowed.  As the reference's caller does, Process of an
 * adaptive-digital stream gets the level VirtualMic returned.
 * mic_level_in == NULL: frame f + 1 of a stream gets the level frame f returned in mic_level_out, the first
 * frame the stream's stored level (after Init, a setter, or the last such call); an adaptive-digital stream
 * keeps its stored level, the static physical level VirtualMic is defined on.  With mic_level_in given the
 * stored levels are left alone.  mic_level_out / saturation may be NULL. */
int AspAgcBatch_ProcessFrames(AspAgcBatch* b, int num_frames, const int16_t* far, const int16_t* low_in,
                              const int16_t* high_in, int16_t* low_out, int16_t* high_out, int num_bands,
                              int samples_per_band, const int32_t* mic_level_in, const int16_t* echo,
                              int32_t* mic_level_out, uint8_t* saturation, int mem);
int AspAgcBatch_returns(AspAgcBatch* b, int32_t* out, int count); /* host int32 [count], count <= frames * streams */
int AspAgcBatch_ExportState(AspAgcBatch* b, int stream, AspAgcState* out);
int AspAgcBatch_ImportState(AspAgcBatch* b, int stream, const AspAgcState* in);
int AspAgcBatch_SetStream(AspAgcBatch* b, void* hip_stream); /* NULL: back to the batch's own stream */
int AspAgcBatch_Synchronize(AspAgcBatch* b);
#ifdef __cplusplus
}
#endif
#endif /* ASP_AGC_H_ */
