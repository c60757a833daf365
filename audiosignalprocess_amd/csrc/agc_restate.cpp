// agc_restate.cpp -- the CPU build of agc_core.h, for the tests only (lib/libagc_restate.so; not part of
// libasp_amd.so, which has no CPU path).  The same source the kernel runs, with a "group" of one lane:
// tests/test_agc_host.py holds it to the golden on machines without a GPU.
#include <stdlib.h>
#include <string.h>

#include "agc_core.h"

using namespace aspagc;

namespace {
struct Inst {
  AspAgcState s;
  AgcWork w;
};
bool good_len(const Inst* p, int n) { return p->s.initFlag == 42 && n == (p->s.fs == 8000 ? 80 : 160); }
}  // namespace

extern "C" {
void* AgcRestate_Create(void) { return calloc(1, sizeof(Inst)); }
void AgcRestate_Free(void* h) { free(h); }
AspAgcState* AgcRestate_State(void* h) { return &((Inst*)h)->s; }

int AgcRestate_Init(void* h, int32_t minLevel, int32_t maxLevel, int16_t mode, uint32_t fs) {
  if (!h || mode < 0 || mode > 3 || (fs != 8000 && fs != 16000 && fs != 32000 && fs != 48000)) return -1;
  return init_core(((Inst*)h)->s, minLevel, maxLevel, mode, fs);
}
int AgcRestate_set_config(void* h, int16_t targetLevelDbfs, int16_t compressionGaindB, uint8_t limiterEnable) {
  return set_config_core(((Inst*)h)->s, targetLevelDbfs, compressionGaindB, limiterEnable);
}
int AgcRestate_gain_table(int32_t* table, int16_t comp, int16_t target, uint8_t limiter, int16_t analogTarget) {
  return calculate_gain_table(table, comp, target, limiter, analogTarget);
}

// One frame of the operations in `ops` (agc_core.h kOp*).  bands: nb pointers to n samples, read and, unless
// out is given, written back; out: nb pointers or NULL.  io: level_in, echo in; vm_level, level_out,
// saturation out.  Returns the reference's return value.
int AgcRestate_Frame(void* h, int ops, const int16_t* far, int16_t* const* bands, int nb, int n, int16_t* const* out,
                     int32_t level_in, int16_t echo, int32_t* vm_level, int32_t* level_out, uint8_t* saturation) {
  Inst* p = (Inst*)h;
  if (!p || !good_len(p, n) || nb < 1 || nb > 3) return -1;
  if (far) memcpy(p->w.far, far, n * sizeof(int16_t));
  for (int b = 0; bands && b < nb; ++b) memcpy(p->w.x[b], bands[b], n * sizeof(int16_t));
  FrameIo io = {level_in, echo, level_in, level_in, 0, 0};
  frame_core<1>(p->s, p->w, ops, nb, n, io, Grp<1>{0});
  for (int b = 0; bands && b < nb; ++b) memcpy(out ? out[b] : bands[b], p->w.x[b], n * sizeof(int16_t));
  if (vm_level) *vm_level = io.vm_level;
  if (level_out) *level_out = io.level_out;
  if (saturation) *saturation = io.saturation;
  return io.rc;
}
}
