// ts_api.hip -- host side of include/asp_ts.h: the batch handle (per stream an AspTsState and the buffer array
// in [C][N], out [C][N], mean [C][bins] in HBM), the Create- and Initialize-time tables (ts_core.h's own
// evaluations; libm is not called), Suppress's argument checks, staging for host-memory callers.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "api_common.h"
#include "ts_core.h"

namespace aspts {
hipError_t launch_suppress(const TsConfig& c, const TsTables& tb, AspTsState* states, float* bufs, size_t stride, int S,
                           int F, float* data, const float* det, const float* ref, int ref_len, const uint8_t* present,
                           const float* voice, const uint8_t* keys, int32_t* results, int* errors, hipStream_t stream);
}  // namespace aspts

using namespace aspts;

#define ts_fail(...) asp_fail("asp_ts", __VA_ARGS__)
#define TS_TRY(x) ASP_TRY("asp_ts", x)

struct AspTsBatch {
  int S = 0, device = 0;
  bool ready = false;
  TsConfig c{};
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspTsState* states = nullptr;  // [S]
  float* bufs = nullptr;         // [S][stride]
  size_t stride = 0;
  float* phase = nullptr;        // [kPhases][2]
  float* tables = nullptr;       // window [N], w [N / 2], mean_factor [bins]
  int* errors = nullptr;
  AspStage s_data, s_det, s_ref, s_present, s_voice, s_keys, s_results;  // staging for host-memory callers
};

namespace {
int table_length(int which, int n) { return which == 0 ? n : which == 1 ? n / 2 : which == 2 ? n / 2 + 1 : -1; }

void make_table(int which, int n, float* out) {
  if (which == 0) make_window(n, out);
  if (which == 1) make_fft_w(n, out);
  if (which == 2) make_mean_factor(n / 2 + 1, out);
}

int init_streams(AspTsBatch* b, int first, int count) {
  AspTsState st;
  memset(&st, 0, sizeof st);
  init_state(st, b->c);
  std::vector<AspTsState> all((size_t)count, st);
  TS_TRY(hipMemcpyAsync(b->states + first, all.data(), sizeof(AspTsState) * (size_t)count, hipMemcpyHostToDevice,
                        b->stream));
  TS_TRY(hipMemsetAsync(b->bufs + (size_t)first * b->stride, 0, sizeof(float) * b->stride * (size_t)count, b->stream));
  TS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int run(AspTsBatch* b, int F, float* data, size_t data_length, int num_channels, const float* det,
        size_t detection_length, const float* ref, size_t reference_length, const uint8_t* present, const float* voice,
        const uint8_t* keys, int32_t* results, int mem) {
  if (!b || (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE) || F < 0) return ASP_ERR_PARAM;
  const TsConfig& c = b->c;
  // TransientSuppressor::Suppress's checks (an uninitialised instance has every length 0)
  if (!b->ready || !data || data_length != (size_t)c.L || num_channels != c.C || detection_length != (size_t)c.D)
    return -1;
  if (!det && c.D > c.L) return -1;  // the reference would read past in_buffer_'s newest chunk
  if (!voice || !keys) return ASP_ERR_PARAM;
  if (reference_length > (size_t)INT32_MAX) return ASP_ERR_PARAM;
  if (F == 0) return 0;
  AspDeviceScope dev_scope_;
  TS_TRY(dev_scope_.select(b->device));
  const size_t U = (size_t)F * b->S;
  const size_t nb_data = U * c.C * c.L * sizeof(float), nb_det = U * c.D * sizeof(float);
  const size_t nb_ref = U * reference_length * sizeof(float);
  float* d_data = data;
  const float *d_det = det, *d_ref = ref, *d_voice = voice;
  const uint8_t *d_present = ref ? present : nullptr, *d_keys = keys;
  int32_t* d_results = results;
  if (mem == ASP_MEM_HOST) {
    struct Up { AspStage* st; const void* src; size_t bytes; const void** dst; };
    Up ups[] = {{&b->s_data, data, nb_data, (const void**)&d_data}, {&b->s_det, det, nb_det, (const void**)&d_det},
                {&b->s_ref, ref, nb_ref, (const void**)&d_ref}, {&b->s_present, d_present, U, (const void**)&d_present},
                {&b->s_voice, voice, U * sizeof(float), (const void**)&d_voice}, {&b->s_keys, keys, U, (const void**)&d_keys}};
    for (const Up& u : ups) {
      if (!u.src) continue;
      TS_TRY(u.st->reserve(u.bytes ? u.bytes : 4));
      if (u.bytes) TS_TRY(hipMemcpyAsync(u.st->p, u.src, u.bytes, hipMemcpyHostToDevice, b->stream));
      *u.dst = u.st->p;
    }
    TS_TRY(b->s_results.reserve(U * sizeof(int32_t)));
    d_results = (int32_t*)b->s_results.p;
  }
  if (ref && reference_length == 0) d_ref = d_data;  // never read (no samples), but a reference all the same
  TS_TRY(hipMemsetAsync(b->errors, 0, sizeof(int), b->stream));
  const TsTables tb{b->tables, b->tables + c.N, b->tables + c.N + c.N / 2, b->phase};
  TS_TRY(launch_suppress(c, tb, b->states, b->bufs, b->stride, b->S, F, d_data, d_det, d_ref, (int)reference_length,
                         d_present, d_voice, d_keys, d_results, b->errors, b->stream));
  int errors = 0;
  TS_TRY(hipMemcpyAsync(&errors, b->errors, sizeof(int), hipMemcpyDeviceToHost, b->stream));
  if (mem == ASP_MEM_HOST) {
    TS_TRY(hipMemcpyAsync(data, d_data, nb_data, hipMemcpyDeviceToHost, b->stream));
    if (results) TS_TRY(hipMemcpyAsync(results, d_results, U * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
  }
  TS_TRY(hipStreamSynchronize(b->stream));
  return errors ? -1 : 0;
}
}  // namespace

extern "C" {

size_t AspTs_state_size(void) { return sizeof(AspTsState); }

int AspTs_table(int which, int n, float* out, int cap) {
  if (!out || (n != 128 && n != 256 && n != 512 && n != 1024)) return ASP_ERR_PARAM;
  const int len = table_length(which, n);
  if (len < 0 || cap < len) return ASP_ERR_PARAM;
  make_table(which, n, out);
  return len;
}

int AspTsBatch_Free(AspTsBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
  void* bufs[] = {b->states, b->bufs, b->phase, b->tables, b->errors, b->s_data.p, b->s_det.p, b->s_ref.p,
                  b->s_present.p, b->s_voice.p, b->s_keys.p, b->s_results.p};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspTsBatch_Create(AspTsBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return ts_fail(ASP_ERR_PARAM, "AspTsBatch_Create: NULL out or num_streams < 1");
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_ts", device, ASP_ERR_NO_DEVICE, "AspTsBatch_Create: no HIP device")) return rc;
  AspTsBatch* b = new AspTsBatch;
  b->S = num_streams;
  b->device = device;
  std::vector<float> phase(2 * (size_t)kPhases);
  make_phase(phase.data());
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->states, sizeof(AspTsState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMalloc((void**)&b->phase, sizeof(float) * phase.size());
  if (e == hipSuccess) e = hipMalloc((void**)&b->tables, sizeof(float) * (kMaxN + kMaxN / 2 + kMaxBins));
  if (e == hipSuccess) e = hipMalloc((void**)&b->errors, sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(b->phase, phase.data(), sizeof(float) * phase.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    AspTsBatch_Free(b);
    return ts_fail(ASP_ERR_HIP, "AspTsBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspTsBatch_num_streams(const AspTsBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspTsBatch_Initialize(AspTsBatch* b, int sample_rate_hz, int detection_rate_hz, int num_channels) {
  if (!b) return ASP_ERR_PARAM;
  TsConfig c;
  if (!make_config(c, sample_rate_hz, detection_rate_hz, num_channels)) return -1;
  AspDeviceScope dev_scope_;
  TS_TRY(dev_scope_.select(b->device));
  TS_TRY(hipStreamSynchronize(b->stream));
  const size_t stride = buffer_floats(c);
  if (stride != b->stride || !b->bufs) {
    b->ready = false;
    if (b->bufs) (void)hipFree(b->bufs);
    b->bufs = nullptr;
    TS_TRY(hipMalloc((void**)&b->bufs, sizeof(float) * stride * (size_t)b->S));
    b->stride = stride;
  }
  b->c = c;
  std::vector<float> t((size_t)c.N + c.N / 2 + c.bins);
  make_table(0, c.N, t.data());
  make_table(1, c.N, t.data() + c.N);
  make_table(2, c.N, t.data() + c.N + c.N / 2);
  TS_TRY(hipMemcpy(b->tables, t.data(), sizeof(float) * t.size(), hipMemcpyHostToDevice));
  if (int rc = init_streams(b, 0, b->S)) return rc;
  b->ready = true;
  return 0;
}

int AspTsBatch_InitializeStream(AspTsBatch* b, int stream) {
  if (!b || stream < 0 || stream >= b->S) return ASP_ERR_PARAM;
  if (!b->ready) return -1;
  AspDeviceScope dev_scope_;
  TS_TRY(dev_scope_.select(b->device));
  return init_streams(b, stream, 1);
}

int AspTsBatch_state_floats(const AspTsBatch* b) { return b && b->ready ? (int)b->stride : -1; }

int AspTsBatch_GetState(AspTsBatch* b, int stream, AspTsState* state, float* buffers) {
  if (!b || stream < 0 || stream >= b->S || !state || !buffers) return ASP_ERR_PARAM;
  if (!b->ready) return ts_fail(ASP_ERR_STATE, "AspTsBatch_GetState: not initialised");
  AspDeviceScope dev_scope_;
  TS_TRY(dev_scope_.select(b->device));
  TS_TRY(hipMemcpyAsync(state, b->states + stream, sizeof(AspTsState), hipMemcpyDeviceToHost, b->stream));
  TS_TRY(hipMemcpyAsync(buffers, b->bufs + (size_t)stream * b->stride, sizeof(float) * b->stride, hipMemcpyDeviceToHost,
                        b->stream));
  TS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspTsBatch_SetState(AspTsBatch* b, int stream, const AspTsState* state, const float* buffers) {
  if (!b || stream < 0 || stream >= b->S || !state || !buffers) return ASP_ERR_PARAM;
  if (!b->ready) return ts_fail(ASP_ERR_STATE, "AspTsBatch_SetState: not initialised");
  if (state->sample_rate_hz != b->c.rate || state->detection_rate_hz != b->c.det_rate ||
      state->num_channels != b->c.C || state->queue_pos < 0 || state->queue_pos > 2)
    return ts_fail(ASP_ERR_PARAM, "AspTsBatch_SetState: the state's rates or channels are not the batch's");
  AspDeviceScope dev_scope_;
  TS_TRY(dev_scope_.select(b->device));
  TS_TRY(hipMemcpyAsync(b->states + stream, state, sizeof(AspTsState), hipMemcpyHostToDevice, b->stream));
  TS_TRY(hipMemcpyAsync(b->bufs + (size_t)stream * b->stride, buffers, sizeof(float) * b->stride, hipMemcpyHostToDevice,
                        b->stream));
  TS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspTsBatch_Suppress(AspTsBatch* b, float* data, size_t data_length, int num_channels, const float* detection_data,
                        size_t detection_length, const float* reference_data, size_t reference_length,
                        const uint8_t* reference_present, const float* voice_probability, const uint8_t* key_pressed,
                        int32_t* results, int mem) {
  return run(b, 1, data, data_length, num_channels, detection_data, detection_length, reference_data, reference_length,
             reference_present, voice_probability, key_pressed, results, mem);
}

int AspTsBatch_SuppressFrames(AspTsBatch* b, int num_frames, float* data, size_t data_length, int num_channels,
                              const float* detection_data, size_t detection_length, const float* reference_data,
                              size_t reference_length, const uint8_t* reference_present,
                              const float* voice_probability, const uint8_t* key_pressed, int32_t* results, int mem) {
  return run(b, num_frames, data, data_length, num_channels, detection_data, detection_length, reference_data,
             reference_length, reference_present, voice_probability, key_pressed, results, mem);
}

int AspTsBatch_SetStream(AspTsBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspTsBatch_Synchronize(AspTsBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  TS_TRY(dev_scope_.select(b->device));
  TS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

}  // extern "C"
