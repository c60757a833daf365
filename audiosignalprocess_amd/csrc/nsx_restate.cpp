// nsx_restate.cpp -- the CPU build of nsx_core.h, for the tests only (lib/libnsx_restate.so; not part of
// libasp_amd.so, which has no CPU path).  The same source the kernel runs, with one "lane" that walks
// every bin: tests/test_nsx_host.py holds it to the golden on machines without a GPU.
#include <stdlib.h>

#include "nsx_core.h"

using namespace aspnsx;

namespace {
struct Inst {
  AspNsxState s;
  NsxWork w;
  NsxTables T;
};
}  // namespace

extern "C" {
void* NsxRestate_Create(void) {
  Inst* p = (Inst*)calloc(1, sizeof(Inst));
  if (p) build_tables(&p->T);
  return p;
}
void NsxRestate_Free(void* h) { free(h); }
int NsxRestate_Init(void* h, uint32_t fs) { return init_core(((Inst*)h)->s, fs); }
int NsxRestate_set_policy(void* h, int mode) { return set_policy_core(((Inst*)h)->s, mode); }
int NsxRestate_Process(void* h, const int16_t* const* in, int num_bands, int16_t* const* out) {
  Inst* p = (Inst*)h;
  if (p->s.initFlag != 1 || num_bands < 1 || num_bands > 3) return -1;
  process_core(p->s, p->w, p->s.histLrt, in, num_bands, out, p->T, Lanes{0, 1});
  return 0;
}
AspNsxState* NsxRestate_State(void* h) { return &((Inst*)h)->s; }
const NsxTables* NsxRestate_Tables(void* h) { return &((Inst*)h)->T; }
}
