// hpf_restate.cpp -- the CPU build of hpf_core.h and level_core.h, for the tests only (lib/libhpf_restate.so; not
// part of libasp_amd.so, which has no CPU path).  The same sources the kernels run, one stream-channel (filter) or
// one stream (meter) at a time: tests/test_hpf_host.py holds it to the golden on machines without a GPU.
#include <stdlib.h>

#include "hpf_core.h"
#include "level_core.h"

using namespace asphpf;

extern "C" {
void* HpfRestate_Create(void) { return calloc(1, sizeof(AspHpfState)); }
void HpfRestate_Free(void* h) { free(h); }
AspHpfState* HpfRestate_State(void* h) { return (AspHpfState*)h; }

int HpfRestate_Init(void* h, int sample_rate_hz) {
  const int set = coeff_set_of_rate(sample_rate_hz);
  if (!h || set < 0) return -1;
  init_state(*(AspHpfState*)h, set);
  return 0;
}

// Filter, in place
int HpfRestate_Process(void* h, int16_t* data, int length) {
  if (!h || !data || length < 0) return -1;
  AspHpfState& s = *(AspHpfState*)h;
  HpfRegs r = load_regs(s);
  const HpfCoeffs c = coeffs(s.coeff_set);
  for (int i = 0; i < length; ++i) data[i] = (int16_t)filter_sample(r, c, data[i]);
  store_regs(s, r);
  return 0;
}

// FloatS16ToS16, Filter, back to float, in place
int HpfRestate_ProcessFloatS16(void* h, float* data, int length) {
  if (!h || !data || length < 0) return -1;
  AspHpfState& s = *(AspHpfState*)h;
  HpfRegs r = load_regs(s);
  const HpfCoeffs c = coeffs(s.coeff_set);
  for (int i = 0; i < length; ++i) data[i] = (float)(int16_t)filter_sample(r, c, float_s16_to_s16(data[i]));
  store_regs(s, r);
  return 0;
}

void* LevelRestate_Create(void) { return calloc(1, sizeof(AspLevelState)); }
void LevelRestate_Free(void* h) { free(h); }
AspLevelState* LevelRestate_State(void* h) { return (AspLevelState*)h; }
void LevelRestate_Reset(void* h) { *(AspLevelState*)h = AspLevelState{0.f, 0}; }

void LevelRestate_Process(void* h, const int16_t* data, int length) {
  AspLevelState& s = *(AspLevelState*)h;
  for (int i = 0; i < length; ++i) level_add(s.sum_square, data[i]);
  level_count(s, length);
}

void LevelRestate_ProcessMuted(void* h, int length) { level_count(*(AspLevelState*)h, length); }
int LevelRestate_RMS(void* h) { return level_rms(*(AspLevelState*)h); }
}
