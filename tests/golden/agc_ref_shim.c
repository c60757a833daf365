/* agc_ref_shim.c -- golden generation only (tests/golden/make_agc_golden.py): built together with the
 * reference's analog_agc.c / digital_agc.c, gives the generator an instance that is all zero before Init
 * (WebRtcAgc_Init leaves some fields as malloc gave them) and copies a LegacyAgc, field by field, into the
 * flat AspAgcState of include/asp_agc.h. */
#include <string.h>

#include "webrtc/modules/audio_processing/agc/legacy/analog_agc.h"

#include "asp_agc.h"

void* agc_ref_create(void) {
  void* h = NULL;
  if (WebRtcAgc_Create(&h) != 0) return NULL;
  memset(h, 0, sizeof(LegacyAgc));
  return h;
}

size_t agc_ref_sizeof(void) { return sizeof(LegacyAgc); }

/* the seeded cases of tests/agc_runs.py: one scalar field of the instance by name; -1 for a name not listed */
int agc_ref_set(void* h, const char* name, int value) {
  LegacyAgc* a = (LegacyAgc*)h;
#define SET(f) if (strcmp(name, #f) == 0) { a->f = value; return 0; }
  SET(msZero) SET(zeroCtrlMax)
#undef SET
  return -1;
}

#define COPY(f) o->f = a->f
#define COPY_ARR(f) memcpy(o->f, a->f, sizeof o->f)
#define COPY_VAD(dst, src)                                        \
  memcpy(o->dst##_downState, (src).downState, sizeof(src).downState); \
  o->dst##_HPstate = (src).HPstate;                               \
  o->dst##_counter = (src).counter;                               \
  o->dst##_logRatio = (src).logRatio;                             \
  o->dst##_meanLongTerm = (src).meanLongTerm;                     \
  o->dst##_varianceLongTerm = (src).varianceLongTerm;             \
  o->dst##_stdLongTerm = (src).stdLongTerm;                       \
  o->dst##_meanShortTerm = (src).meanShortTerm;                   \
  o->dst##_varianceShortTerm = (src).varianceShortTerm;           \
  o->dst##_stdShortTerm = (src).stdShortTerm

void agc_ref_state(const void* h, AspAgcState* o) {
  const LegacyAgc* a = (const LegacyAgc*)h;
  memset(o, 0, sizeof *o);
  COPY(fs); COPY(compressionGaindB); COPY(targetLevelDbfs); COPY(agcMode); COPY(limiterEnable);
  o->defaultConfig_targetLevelDbfs = a->defaultConfig.targetLevelDbfs;
  o->defaultConfig_compressionGaindB = a->defaultConfig.compressionGaindB;
  o->defaultConfig_limiterEnable = a->defaultConfig.limiterEnable;
  o->usedConfig_targetLevelDbfs = a->usedConfig.targetLevelDbfs;
  o->usedConfig_compressionGaindB = a->usedConfig.compressionGaindB;
  o->usedConfig_limiterEnable = a->usedConfig.limiterEnable;
  COPY(initFlag); COPY(lastError);
  COPY(analogTargetLevel); COPY(startUpperLimit); COPY(startLowerLimit); COPY(upperPrimaryLimit);
  COPY(lowerPrimaryLimit); COPY(upperSecondaryLimit); COPY(lowerSecondaryLimit); COPY(targetIdx);
  COPY(analogTarget); COPY_ARR(filterState); COPY(upperLimit); COPY(lowerLimit); COPY(Rxx160w32);
  COPY(Rxx16_LPw32); COPY(Rxx160_LPw32); COPY(Rxx16_LPw32Max); COPY_ARR(Rxx16_vectorw32);
  COPY_ARR(Rxx16w32_array); COPY_ARR(env);
  COPY(Rxx16pos); COPY(envSum); COPY(vadThreshold); COPY(inActive); COPY(msTooLow); COPY(msTooHigh);
  COPY(changeToSlowMode); COPY(firstCall); COPY(msZero); COPY(msecSpeechOuterChange);
  COPY(msecSpeechInnerChange); COPY(activeSpeech); COPY(muteGuardMs); COPY(inQueue);
  COPY(micRef); COPY(gainTableIdx); COPY(micGainIdx); COPY(micVol); COPY(maxLevel); COPY(maxAnalog);
  COPY(maxInit); COPY(minLevel); COPY(minOutput); COPY(zeroCtrlMax); COPY(lastInMicLevel); COPY(scale);
  COPY_VAD(vadMic, a->vadMic);
  o->digitalAgc_capacitorSlow = a->digitalAgc.capacitorSlow;
  o->digitalAgc_capacitorFast = a->digitalAgc.capacitorFast;
  o->digitalAgc_gain = a->digitalAgc.gain;
  memcpy(o->digitalAgc_gainTable, a->digitalAgc.gainTable, sizeof o->digitalAgc_gainTable);
  o->digitalAgc_gatePrevious = a->digitalAgc.gatePrevious;
  o->digitalAgc_agcMode = a->digitalAgc.agcMode;
  COPY_VAD(vadNearend, a->digitalAgc.vadNearend);
  COPY_VAD(vadFarend, a->digitalAgc.vadFarend);
  COPY(lowLevelSignal);
}
