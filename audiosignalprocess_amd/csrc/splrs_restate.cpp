// splrs_restate.cpp -- the CPU build of splrs_core.h, for the tests only (lib/libsplrs_restate.so; not part
// of libasp_amd.so, which has no CPU path).  The same source the kernel runs, with one "lane" per channel:
// tests/test_splrs_host.py holds it to the golden on machines without a GPU.  An instance is one channel
// (kResamplerSynchronous); the tests pair two for the stereo run, as the reference pairs two slaves.
#include <stdlib.h>
#include <string.h>

#include "splrs_core.h"

using namespace aspsplrs;

extern "C" {
void* SplrsRestate_Create(void) {
  AspResamplerState* p = (AspResamplerState*)calloc(1, sizeof(AspResamplerState));
  if (p) p->mode = -1;
  return p;
}
void SplrsRestate_Free(void* h) { free(h); }
int SplrsRestate_Reset(void* h, int in_freq, int out_freq) {
  AspResamplerState* p = (AspResamplerState*)h;
  memset(p, 0, sizeof *p);
  p->in_freq_khz = in_freq / 1000;
  p->out_freq_khz = out_freq / 1000;
  p->mode = select_mode(in_freq, out_freq);
  return p->mode < 0 ? -1 : 0;
}
int SplrsRestate_Push(void* h, const int16_t* in, int length_in, int16_t* out, int max_len, int* out_len) {
  AspResamplerState* p = (AspResamplerState*)h;
  const int olen = check_push(p->mode, length_in, max_len);
  if (olen < 0) return -1;
  int16_t a[kPieceMax], b[kPieceMax];
  int32_t w[kWork];
  const int piece = kChain[p->mode].piece;
  int done = 0;
  for (int off = 0; off < length_in; off += piece) {
    const int n = length_in - off < piece ? length_in - off : piece;
    memcpy(a, in + off, n * sizeof(int16_t));
    int16_t* res;
    const int m = push_piece<1>(p->mode, &p->stage[0][0], a, n, b, w, 0, &res);
    memcpy(out + done, res, m * sizeof(int16_t));
    done += m;
  }
  *out_len = olen;
  return 0;
}
AspResamplerState* SplrsRestate_State(void* h) { return (AspResamplerState*)h; }
}
