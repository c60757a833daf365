// level_api.hip -- host side of include/asp_level.h: the batch handle (per stream an AspLevelState in HBM),
// Process's argument checks, staging for host-memory callers, and RMS(), which reads the accumulators back and
// evaluates level_core.h's level_rms on the host.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "api_common.h"
#include "level_core.h"

namespace asphpf {
struct LevelArgs {
  AspLevelState* state;
  int S, F, row;
  const int16_t* in;
};
hipError_t launch_level(const LevelArgs& a, hipStream_t stream);
hipError_t launch_level_muted(AspLevelState* state, int count, int32_t length, hipStream_t stream);
}  // namespace asphpf

using namespace asphpf;

#define level_fail(...) asp_fail("asp_level", __VA_ARGS__)
#define LEVEL_TRY(x) ASP_TRY("asp_level", x)

struct AspLevelBatch {
  int S = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspLevelState* states = nullptr;  // [S]
  AspStage s_in;                    // staging for host-memory callers
};

namespace {
bool good_stream(const AspLevelBatch* b, int stream) { return b && stream >= 0 && stream < b->S; }

int reset(AspLevelBatch* b, int first, int count) {
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  LEVEL_TRY(hipMemsetAsync(b->states + first, 0, sizeof(AspLevelState) * (size_t)count, b->stream));
  return ASP_OK;
}

int muted(AspLevelBatch* b, int first, int count, int length) {
  if (length < 0) return level_fail(ASP_ERR_PARAM, "AspLevelBatch_ProcessMuted: length < 0");
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  LEVEL_TRY(launch_level_muted(b->states + first, count, length, b->stream));
  return ASP_OK;
}

// RMS() of streams [first, first + count): read back, evaluate, reset
int rms(AspLevelBatch* b, int first, int count, int32_t* out) {
  if (!out) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  std::vector<AspLevelState> st((size_t)count);
  LEVEL_TRY(hipMemcpyAsync(st.data(), b->states + first, sizeof(AspLevelState) * (size_t)count, hipMemcpyDeviceToHost,
                           b->stream));
  LEVEL_TRY(hipMemsetAsync(b->states + first, 0, sizeof(AspLevelState) * (size_t)count, b->stream));
  LEVEL_TRY(hipStreamSynchronize(b->stream));
  for (int s = 0; s < count; ++s) out[s] = level_rms(st[(size_t)s]);
  return ASP_OK;
}
}  // namespace

extern "C" {

size_t AspLevel_state_size(void) { return sizeof(AspLevelState); }

int AspLevelBatch_Free(AspLevelBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->states) (void)hipFree(b->states);
  b->s_in.release();
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspLevelBatch_Create(AspLevelBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return level_fail(ASP_ERR_PARAM, "AspLevelBatch_Create: NULL out or num_streams < 1");
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_level", device, ASP_ERR_NO_DEVICE, "AspLevelBatch_Create: no HIP device"))
    return rc;
  AspLevelBatch* b = new AspLevelBatch;
  b->S = num_streams;
  b->device = device;
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->states, sizeof(AspLevelState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMemset(b->states, 0, sizeof(AspLevelState) * (size_t)num_streams);
  if (e != hipSuccess) {
    AspLevelBatch_Free(b);
    return level_fail(ASP_ERR_HIP, "AspLevelBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspLevelBatch_num_streams(const AspLevelBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspLevelBatch_Reset(AspLevelBatch* b) { return b ? reset(b, 0, b->S) : ASP_ERR_PARAM; }
int AspLevelBatch_ResetStream(AspLevelBatch* b, int stream) {
  return good_stream(b, stream) ? reset(b, stream, 1) : ASP_ERR_PARAM;
}

int AspLevelBatch_Process(AspLevelBatch* b, const int16_t* in, int num_frames, int num_channels, int samples, int mem) {
  if (!b) return ASP_ERR_PARAM;
  if (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE) return level_fail(ASP_ERR_PARAM, "AspLevelBatch_Process: bad mem");
  if (!in || num_frames < 0) return level_fail(ASP_ERR_PARAM, "AspLevelBatch_Process: NULL buffer or num_frames < 0");
  if (num_channels < 1 || num_channels > ASP_LEVEL_MAX_CHANNELS)
    return level_fail(ASP_ERR_PARAM, "AspLevelBatch_Process: num_channels outside 1 .. ASP_LEVEL_MAX_CHANNELS");
  if (samples < 1 || samples > ASP_LEVEL_MAX_SAMPLES)
    return level_fail(ASP_ERR_PARAM, "AspLevelBatch_Process: samples outside 1 .. ASP_LEVEL_MAX_SAMPLES");
  if (num_frames == 0) return ASP_OK;
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  LevelArgs a{b->states, b->S, num_frames, num_channels * samples, in};
  if (mem == ASP_MEM_HOST) {
    const size_t bytes = (size_t)num_frames * b->S * a.row * sizeof(int16_t);
    LEVEL_TRY(b->s_in.reserve(bytes));
    LEVEL_TRY(hipMemcpyAsync(b->s_in.p, in, bytes, hipMemcpyHostToDevice, b->stream));
    a.in = (const int16_t*)b->s_in.p;
  }
  LEVEL_TRY(launch_level(a, b->stream));
  if (mem == ASP_MEM_HOST) LEVEL_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspLevelBatch_ProcessMuted(AspLevelBatch* b, int length) { return b ? muted(b, 0, b->S, length) : ASP_ERR_PARAM; }
int AspLevelBatch_ProcessMutedStream(AspLevelBatch* b, int stream, int length) {
  return good_stream(b, stream) ? muted(b, stream, 1, length) : ASP_ERR_PARAM;
}

int AspLevelBatch_RMS(AspLevelBatch* b, int32_t* out) { return b ? rms(b, 0, b->S, out) : ASP_ERR_PARAM; }
int AspLevelBatch_RMS_stream(AspLevelBatch* b, int stream, int32_t* out) {
  return good_stream(b, stream) ? rms(b, stream, 1, out) : ASP_ERR_PARAM;
}

int AspLevelBatch_ExportState(AspLevelBatch* b, int stream, AspLevelState* state) {
  if (!good_stream(b, stream) || !state) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  LEVEL_TRY(hipMemcpyAsync(state, b->states + stream, sizeof(AspLevelState), hipMemcpyDeviceToHost, b->stream));
  LEVEL_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspLevelBatch_ImportState(AspLevelBatch* b, int stream, const AspLevelState* state) {
  if (!good_stream(b, stream) || !state) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  LEVEL_TRY(hipMemcpyAsync(b->states + stream, state, sizeof(AspLevelState), hipMemcpyHostToDevice, b->stream));
  LEVEL_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspLevelBatch_SetStream(AspLevelBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspLevelBatch_Synchronize(AspLevelBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  LEVEL_TRY(dev_scope_.select(b->device));
  LEVEL_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

}  // extern "C"
