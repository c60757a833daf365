// hpf_api.hip -- host side of include/asp_hpf.h: the batch handle (per stream-channel an AspHpfState in HBM),
// Init's rate checks, Process's argument checks, staging for host-memory callers, the layer-1 handle.  No CPU
// fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "api_common.h"
#include "hpf_core.h"

namespace asphpf {
struct HpfArgs {
  AspHpfState* state;
  int U, F, n;
  const void* in;
  void* out;
};
hipError_t launch_hpf(const HpfArgs& a, bool is_float, hipStream_t stream);
}  // namespace asphpf

using namespace asphpf;

#define hpf_fail(...) asp_fail("asp_hpf", __VA_ARGS__)
#define HPF_TRY(x) ASP_TRY("asp_hpf", x)

struct AspHpfBatch {
  int S = 0, C = 0, device = 0;
  bool ready = false;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspHpfState* states = nullptr;  // [S][C]
  AspStage s_io;                  // staging for host-memory callers
};

struct AspHpf {
  AspHpfBatch* b = nullptr;
};

namespace {
int init_streams(AspHpfBatch* b, int first, int count, int sample_rate_hz, const char* who) {
  const int set = coeff_set_of_rate(sample_rate_hz);
  if (set < 0) return hpf_fail(ASP_ERR_PARAM, who);
  AspHpfState st;
  init_state(st, set);
  std::vector<AspHpfState> all((size_t)count * b->C, st);
  AspDeviceScope dev_scope_;
  HPF_TRY(dev_scope_.select(b->device));
  HPF_TRY(hipMemcpyAsync(b->states + (size_t)first * b->C, all.data(), sizeof(AspHpfState) * all.size(),
                         hipMemcpyHostToDevice, b->stream));
  HPF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int run(AspHpfBatch* b, const void* in, void* out, int F, int n, int mem, bool is_float) {
  if (!b) return ASP_ERR_PARAM;
  if (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE) return hpf_fail(ASP_ERR_PARAM, "AspHpfBatch_Process: bad mem");
  if (!in || !out || F < 0) return hpf_fail(ASP_ERR_PARAM, "AspHpfBatch_Process: NULL buffer or num_frames < 0");
  if (n < 1 || n > ASP_HPF_MAX_SAMPLES)
    return hpf_fail(ASP_ERR_PARAM, "AspHpfBatch_Process: samples outside 1 .. ASP_HPF_MAX_SAMPLES");
  if (!b->ready) return hpf_fail(ASP_ERR_STATE, "AspHpfBatch_Process: not initialised");
  if (F == 0) return ASP_OK;
  AspDeviceScope dev_scope_;
  HPF_TRY(dev_scope_.select(b->device));
  const int U = b->S * b->C;
  const size_t bytes = (size_t)F * U * n * (is_float ? sizeof(float) : sizeof(int16_t));
  HpfArgs a{b->states, U, F, n, in, out};
  if (mem == ASP_MEM_HOST) {
    HPF_TRY(b->s_io.reserve(bytes));
    HPF_TRY(hipMemcpyAsync(b->s_io.p, in, bytes, hipMemcpyHostToDevice, b->stream));
    a.in = a.out = b->s_io.p;
  }
  HPF_TRY(launch_hpf(a, is_float, b->stream));
  if (mem == ASP_MEM_HOST) {
    HPF_TRY(hipMemcpyAsync(out, b->s_io.p, bytes, hipMemcpyDeviceToHost, b->stream));
    HPF_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}

bool good_unit(const AspHpfBatch* b, int stream, int channel) {
  return b && stream >= 0 && stream < b->S && channel >= 0 && channel < b->C;
}
}  // namespace

extern "C" {

size_t AspHpf_state_size(void) { return sizeof(AspHpfState); }

int AspHpfBatch_Free(AspHpfBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->states) (void)hipFree(b->states);
  b->s_io.release();
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspHpfBatch_Create(AspHpfBatch** out, int num_streams, int num_channels, int device) {
  if (!out || num_streams < 1 || num_channels < 1 || (int64_t)num_streams * num_channels > INT32_MAX / 2)
    return hpf_fail(ASP_ERR_PARAM, "AspHpfBatch_Create: NULL out, or num_streams or num_channels < 1");
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_hpf", device, ASP_ERR_NO_DEVICE, "AspHpfBatch_Create: no HIP device")) return rc;
  AspHpfBatch* b = new AspHpfBatch;
  b->S = num_streams;
  b->C = num_channels;
  b->device = device;
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->states, sizeof(AspHpfState) * (size_t)num_streams * num_channels);
  if (e != hipSuccess) {
    AspHpfBatch_Free(b);
    return hpf_fail(ASP_ERR_HIP, "AspHpfBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspHpfBatch_num_streams(const AspHpfBatch* b) { return b ? b->S : ASP_ERR_PARAM; }
int AspHpfBatch_num_channels(const AspHpfBatch* b) { return b ? b->C : ASP_ERR_PARAM; }

int AspHpfBatch_Init(AspHpfBatch* b, int sample_rate_hz) {
  if (!b) return ASP_ERR_PARAM;
  if (int rc = init_streams(b, 0, b->S, sample_rate_hz, "AspHpfBatch_Init: sample rate is not 8000, 16000, 32000 or 48000"))
    return rc;
  b->ready = true;
  return ASP_OK;
}

int AspHpfBatch_InitStream(AspHpfBatch* b, int stream, int sample_rate_hz) {
  if (!b || stream < 0 || stream >= b->S) return ASP_ERR_PARAM;
  if (!b->ready) return hpf_fail(ASP_ERR_STATE, "AspHpfBatch_InitStream: not initialised");
  return init_streams(b, stream, 1, sample_rate_hz,
                      "AspHpfBatch_InitStream: sample rate is not 8000, 16000, 32000 or 48000");
}

int AspHpfBatch_Process(AspHpfBatch* b, const int16_t* in, int16_t* out, int num_frames, int samples, int mem) {
  return run(b, in, out, num_frames, samples, mem, false);
}

int AspHpfBatch_ProcessFloatS16(AspHpfBatch* b, const float* in, float* out, int num_frames, int samples, int mem) {
  return run(b, in, out, num_frames, samples, mem, true);
}

int AspHpfBatch_ExportState(AspHpfBatch* b, int stream, int channel, AspHpfState* state) {
  if (!good_unit(b, stream, channel) || !state) return ASP_ERR_PARAM;
  if (!b->ready) return hpf_fail(ASP_ERR_STATE, "AspHpfBatch_ExportState: not initialised");
  AspDeviceScope dev_scope_;
  HPF_TRY(dev_scope_.select(b->device));
  HPF_TRY(hipMemcpyAsync(state, b->states + (size_t)stream * b->C + channel, sizeof(AspHpfState), hipMemcpyDeviceToHost,
                         b->stream));
  HPF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspHpfBatch_ImportState(AspHpfBatch* b, int stream, int channel, const AspHpfState* state) {
  if (!good_unit(b, stream, channel) || !state) return ASP_ERR_PARAM;
  if (!b->ready) return hpf_fail(ASP_ERR_STATE, "AspHpfBatch_ImportState: not initialised");
  if (state->coeff_set != 0 && state->coeff_set != 1)
    return hpf_fail(ASP_ERR_PARAM, "AspHpfBatch_ImportState: coeff_set is not 0 or 1");
  AspDeviceScope dev_scope_;
  HPF_TRY(dev_scope_.select(b->device));
  HPF_TRY(hipMemcpyAsync(b->states + (size_t)stream * b->C + channel, state, sizeof(AspHpfState), hipMemcpyHostToDevice,
                         b->stream));
  HPF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspHpfBatch_SetStream(AspHpfBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspHpfBatch_Synchronize(AspHpfBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  HPF_TRY(dev_scope_.select(b->device));
  HPF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspHpf_Create(AspHpf** out) {
  if (!out) return ASP_ERR_PARAM;
  *out = nullptr;
  AspHpfBatch* b = nullptr;
  if (int rc = AspHpfBatch_Create(&b, 1, 1, 0)) return rc;
  AspHpf* h = new AspHpf;
  h->b = b;
  *out = h;
  return ASP_OK;
}

int AspHpf_Init(AspHpf* h, int sample_rate_hz) { return h ? AspHpfBatch_Init(h->b, sample_rate_hz) : ASP_ERR_PARAM; }

int AspHpf_Process(AspHpf* h, int16_t* data, int length) {
  return h ? AspHpfBatch_Process(h->b, data, data, 1, length, ASP_MEM_HOST) : ASP_ERR_PARAM;
}

int AspHpf_Free(AspHpf* h) {
  if (!h) return ASP_ERR_PARAM;
  AspHpfBatch_Free(h->b);
  delete h;
  return ASP_OK;
}

}  // extern "C"
