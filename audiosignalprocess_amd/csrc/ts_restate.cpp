// ts_restate.cpp -- the CPU build of ts_core.h, for the tests only (lib/libts_restate.so; not part of
// libasp_amd.so, which has no CPU path).  The same source the kernel runs, with a group of one lane:
// tests/test_ts_host.py holds it to the golden on machines without a GPU.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ts_core.h"

using namespace aspts;

namespace {
struct Tables {
  std::vector<float> window, w, mean_factor;
};
struct Inst {
  bool ready = false;
  TsConfig c;
  AspTsState s;
  TsWork w;
  Tables t;
  std::vector<float> buf;
  TsTables tb;
};
const float* phase_table() {
  static std::vector<float> p;
  if (p.empty()) {
    p.resize(2 * kPhases);
    make_phase(p.data());
  }
  return p.data();
}
}  // namespace

extern "C" {
void* TsRestate_Create(void) { return new Inst; }
void TsRestate_Free(void* h) { delete (Inst*)h; }
AspTsState* TsRestate_State(void* h) { return &((Inst*)h)->s; }
float* TsRestate_Buffers(void* h) { return ((Inst*)h)->buf.data(); }
int TsRestate_BufferFloats(void* h) { return (int)((Inst*)h)->buf.size(); }

int TsRestate_Initialize(void* h, int sample_rate_hz, int detection_rate_hz, int num_channels) {
  Inst* p = (Inst*)h;
  TsConfig c;
  if (!p || !make_config(c, sample_rate_hz, detection_rate_hz, num_channels)) return -1;
  p->c = c;
  p->t.window.resize(c.N);
  p->t.w.resize(c.N / 2);
  p->t.mean_factor.resize(c.bins);
  make_window(c.N, p->t.window.data());
  make_fft_w(c.N, p->t.w.data());
  make_mean_factor(c.bins, p->t.mean_factor.data());
  p->tb = TsTables{p->t.window.data(), p->t.w.data(), p->t.mean_factor.data(), phase_table()};
  p->buf.assign(buffer_floats(c), 0.f);
  init_state(p->s, c);
  p->ready = true;
  return 0;
}

// TransientSuppressor::Suppress's signature
int TsRestate_Suppress(void* h, float* data, size_t data_length, int num_channels, const float* detection_data,
                       size_t detection_length, const float* reference_data, size_t reference_length,
                       float voice_probability, int key_pressed) {
  Inst* p = (Inst*)h;
  if (!p || !p->ready) return -1;
  const TsConfig& c = p->c;
  if (!data || data_length != (size_t)c.L || num_channels != c.C || detection_length != (size_t)c.D) return -1;
  if (!detection_data && c.D > c.L) return -1;  // the reference would read past in_buffer_'s newest chunk
  float* in = p->buf.data();
  float* out = in + (size_t)c.C * c.N;
  float* mean = out + (size_t)c.C * c.N;
  return suppress_chunk(c, p->tb, p->s, p->w, in, out, mean, data, detection_data ? detection_data : data,
                        reference_data, (int)reference_length, voice_probability, key_pressed, Grp{0, 1});
}

// the Create-time tables (include/asp_ts.h AspTs_table) and the core's transcendentals, for the tests
int TsRestate_table(int which, int n, float* out, int cap) {
  if (n != 128 && n != 256 && n != 512 && n != 1024) return -1;
  const int len = which == 0 ? n : which == 1 ? n / 2 : which == 2 ? n / 2 + 1 : -1;
  if (len < 0 || cap < len) return -1;
  if (which == 0) make_window(n, out);
  if (which == 1) make_fft_w(n, out);
  if (which == 2) make_mean_factor(n / 2 + 1, out);
  return len;
}
const float* TsRestate_phase_table(void) { return phase_table(); }
void TsRestate_phases(float* out) { for (int r = 0; r < kPhases; ++r) out[r] = phase_of(r); }
// f: 0 cosf, 1 sinf, 2 expf, 3 powf(x, 50), 4 powf(x, 200)
void TsRestate_eval(int f, const float* x, float* y, size_t n) {
  for (size_t i = 0; i < n; ++i)
    y[i] = f == 0 ? ts_cosf(x[i]) : f == 1 ? ts_sinf(x[i]) : f == 2 ? ts_expf(x[i]) : ts_powf(x[i], f == 3 ? 50.f : 200.f);
}
uint32_t TsRestate_lcg_jump(uint32_t seed, uint32_t k) { return lcg_jump(seed, k); }
}
