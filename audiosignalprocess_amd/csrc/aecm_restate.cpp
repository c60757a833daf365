// aecm_restate.cpp -- the CPU build of aecm_core.h, for the tests only (lib/libaecm_restate.so; not part
// of libasp_amd.so, which has no CPU path).  The same source the kernel runs, one stream per handle:
// tests/test_aecm_host.py holds it to the golden on machines without a GPU.
#include <stdlib.h>

#include "aecm_core.h"

using namespace aspaecm;

namespace {
struct Inst {
  AspAecmState s;
  AecmWork w;
  AecmTables T;
};
}  // namespace

extern "C" {
void* AecmRestate_Create(void) {
  Inst* p = (Inst*)calloc(1, sizeof(Inst));
  if (p) build_tables(&p->T);
  return p;
}
void AecmRestate_Free(void* h) { free(h); }
void AecmRestate_Init(void* h, int fs) { init_instance(((Inst*)h)->s, fs, ((Inst*)h)->T); }
void AecmRestate_SetConfig(void* h, int cng, int echo) { set_config(((Inst*)h)->s, cng, echo); }
void AecmRestate_InitEchoPath(void* h, const int16_t* p) { init_echo_path_core(((Inst*)h)->s, p); }
void AecmRestate_BufferFarend(void* h, const int16_t* far, int n) { buffer_farend(((Inst*)h)->s, far, n); }
void AecmRestate_Process(void* h, const int16_t* nearN, const int16_t* nearC, int16_t* out, int n, int ms) {
  Inst* p = (Inst*)h;
  process(p->s, p->w, nearN, nearC, out, n, ms, p->T);
}
const AspAecmState* AecmRestate_State(void* h) { return &((Inst*)h)->s; }
const AecmTables* AecmRestate_Tables(void* h) { return &((Inst*)h)->T; }
}
