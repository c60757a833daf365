// bf_restate.cpp -- the CPU build of bf_core.h, for the tests only (lib/libbf_restate.so; not part of
// libasp_amd.so, which has no CPU path).  The same source the kernel runs, with a group of one lane:
// tests/test_bf_host.py holds it to the golden on machines without a GPU.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bf_core.h"

using namespace aspbf;

namespace {
struct Inst {
  bool ready = false;
  BfParams p{};
  HostTables h;
  std::vector<float> pack, buf;
  AspBfState s;
  char why[256] = {0};
};

template <int M>
void chunk(Inst* q, const float* input, const float* high, float* output, float* high_output) {
  BfWork<M> w;
  const BfTables tb = view_tables(q->pack.data(), M);
  float* in = q->buf.data();
  process_chunk<M>(q->p, tb, q->s, w, in, in + (size_t)M * kBuf, input, high, output, high_output, Grp{0, 1});
}
}  // namespace

extern "C" {
void* BfRestate_Create(void) { return new Inst; }
void BfRestate_Free(void* h) { delete (Inst*)h; }
AspBfState* BfRestate_State(void* h) { return &((Inst*)h)->s; }
float* BfRestate_Buffers(void* h) { return ((Inst*)h)->buf.data(); }
int BfRestate_BufferFloats(void* h) { return (int)((Inst*)h)->buf.size(); }
const char* BfRestate_Why(void* h) { return ((Inst*)h)->why; }

// the Beamformer constructor and Initialize; -1 with BfRestate_Why() where the call is refused
int BfRestate_Initialize(void* h, int num_mics, const float* geometry_xyz, int chunk_size_ms, int sample_rate_hz) {
  Inst* q = (Inst*)h;
  if (!q) return -1;
  q->ready = false;
  if (const char* why = make_tables(q->h, q->p, num_mics, geometry_xyz, chunk_size_ms, sample_rate_hz)) {
    strncpy(q->why, why, sizeof q->why - 1);
    return -1;
  }
  pack_tables(q->h, q->pack);
  q->buf.assign(buffer_floats(q->p.M), 0.f);
  init_state(q->s, q->p.M, q->p.hold);
  q->ready = true;
  return 0;
}

// input [M][160], high [M][160] or NULL, output [160], high_output [160]; returns is_target_present, or -1
int BfRestate_ProcessChunk(void* h, const float* input, const float* high, float* output, float* high_output) {
  Inst* q = (Inst*)h;
  if (!q || !q->ready || !input || !output || (high && !high_output)) return -1;
  switch (q->p.M) {
    case 2: chunk<2>(q, input, high, output, high_output); break;
    case 3: chunk<3>(q, input, high, output, high_output); break;
    case 4: chunk<4>(q, input, high, output, high_output); break;
    case 5: chunk<5>(q, input, high, output, high_output); break;
    case 6: chunk<6>(q, input, high, output, high_output); break;
    case 7: chunk<7>(q, input, high, output, high_output); break;
    case 8: chunk<8>(q, input, high, output, high_output); break;
    default: return -1;
  }
  return q->s.is_target_present;
}

// the tables in the reference's order (include/asp_bf.h); returns the count, or -1
int BfRestate_GetTables(void* h, int which, float* out, int cap) {
  Inst* q = (Inst*)h;
  if (!q || !q->ready || which < 0 || which >= kTabCount) return -1;
  const std::vector<float>& t = q->h.t[which];
  if (cap < (int)t.size()) return -1;
  memcpy(out, t.data(), sizeof(float) * t.size());
  return (int)t.size();
}
int BfRestate_SetTables(void* h, int which, const float* in, int count) {
  Inst* q = (Inst*)h;
  if (!q || !q->ready || which < 0 || which >= kTabCount || count != table_length(which, q->p.M)) return -1;
  q->h.t[which].assign(in, in + count);
  if (which == kTabDecay) q->p.decay = in[0];
  pack_tables(q->h, q->pack);
  return 0;
}
// mid lower, mid upper, high lower, high upper, hold_target_blocks_
void BfRestate_Params(void* h, int32_t* out) {
  const BfParams& p = ((Inst*)h)->p;
  out[0] = p.mid_lo; out[1] = p.mid_hi; out[2] = p.high_lo; out[3] = p.high_hi; out[4] = p.hold;
}
float BfRestate_MicSpacing(void* h) { return ((Inst*)h)->h.mic_spacing; }
void BfRestate_hypotf(const float* x, const float* y, float* out, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = bf_hypotf(x[i], y[i]);
}
}
