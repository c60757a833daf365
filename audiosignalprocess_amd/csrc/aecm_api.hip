// aecm_api.hip -- host side of include/asp_aecm.h: the batch handle (every stream's AspAecmState and
// AecmWork in HBM), the per-call validation of echo_control_mobile.c (error codes, the msInSndCardBuf
// clamp), the constant tables, and the reference's WebRtcAecm_* as a batch of one stream.
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "aecm_layout.h"
#include "api_common.h"

namespace aspaecm {
hipError_t launch_frames(AspAecmState* st, AecmWork* wk, const AecmTables* T, int S, int F, int n,
                         const int16_t* far, const int16_t* near, const int16_t* clean, int16_t* out,
                         const int16_t* ms, hipStream_t stream);
hipError_t launch_control(AspAecmState* st, const AecmTables* T, int first, int count, int op, int arg,
                          const int16_t* path, hipStream_t stream);
}  // namespace aspaecm

using namespace aspaecm;

#define aecm_fail(...) asp_fail("asp_aecm", __VA_ARGS__)
#define AECM_TRY(x) ASP_TRY("asp_aecm", x)

struct AspAecmBatch {
  int S = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspAecmState* state = nullptr;  // [S]
  AecmWork* work = nullptr;       // [S]
  AecmTables* tables = nullptr;
  std::vector<unsigned char> inited;  // initFlag == 42, per stream
  std::vector<int32_t> last_error;    // lastError, per stream
  std::vector<int16_t> cng, echo;     // the configuration, per stream (get_config)
  std::vector<int16_t> ms_host;       // clamped msInSndCardBuf staging
  AspStage s_far, s_near, s_clean, s_out, s_ms, s_path;  // staging for host-memory callers
};

namespace {
int check_stream(AspAecmBatch* b, int s) { return (b && s >= 0 && s < b->S) ? ASP_OK : ASP_ERR_PARAM; }

int control(AspAecmBatch* b, int first, int count, int op, int arg, const int16_t* path_host) {
  AspDeviceScope dev_scope_;
  AECM_TRY(dev_scope_.select(b->device));
  const int16_t* path = nullptr;
  if (path_host) {
    AECM_TRY(b->s_path.reserve(65 * sizeof(int16_t)));
    AECM_TRY(hipMemcpyAsync(b->s_path.p, path_host, 65 * sizeof(int16_t), hipMemcpyHostToDevice, b->stream));
    path = (const int16_t*)b->s_path.p;
  }
  AECM_TRY(launch_control(b->state, b->tables, first, count, op, arg, path, b->stream));
  if (path_host) AECM_TRY(hipStreamSynchronize(b->stream));  // the staging buffer is reused
  return ASP_OK;
}

// far / near / clean / out: [F][S][n]; ms: [F][S] as given (clamped here); ret: [F][S] or NULL
int run_frames(AspAecmBatch* b, int F, const int16_t* far, const int16_t* near, const int16_t* clean, int16_t* out,
               int n, const int16_t* ms, int32_t* ret, int mem) {
  if (!b || F < 0 || (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE)) return ASP_ERR_PARAM;
  if (n != 80 && n != 160) return ASP_ERR_PARAM;
  if (near && (!out || !ms)) return ASP_ERR_PARAM;
  if (F == 0 || (!far && !near)) return ASP_OK;
  for (int s = 0; s < b->S; ++s)
    if (!b->inited[s]) return aecm_fail(ASP_ERR_STATE, "AspAecmBatch: stream not initialised");
  const int S = b->S;
  const size_t frames = (size_t)F * S, bytes = frames * n * sizeof(int16_t);
  if (near) {
    b->ms_host.resize(frames);
    for (size_t i = 0; i < frames; ++i) {
      int v = ms[i], r = 0;
      if (v < 0) {
        v = 0;
        r = -1;
      } else if (v > 500) {
        v = 500;
        r = -1;
      }
      if (r) b->last_error[i % S] = AECM_BAD_PARAMETER_WARNING;
      b->ms_host[i] = (int16_t)v;
      if (ret) ret[i] = r;
    }
  }
  AspDeviceScope dev_scope_;
  AECM_TRY(dev_scope_.select(b->device));
  const int16_t *d_far = far, *d_near = near, *d_clean = clean;
  int16_t* d_out = out;
  if (mem == ASP_MEM_HOST) {
    if (far) {
      AECM_TRY(b->s_far.reserve(bytes));
      AECM_TRY(hipMemcpyAsync(b->s_far.p, far, bytes, hipMemcpyHostToDevice, b->stream));
      d_far = (const int16_t*)b->s_far.p;
    }
    if (near) {
      AECM_TRY(b->s_near.reserve(bytes));
      AECM_TRY(hipMemcpyAsync(b->s_near.p, near, bytes, hipMemcpyHostToDevice, b->stream));
      d_near = (const int16_t*)b->s_near.p;
      AECM_TRY(b->s_out.reserve(bytes));
      d_out = (int16_t*)b->s_out.p;
    }
    if (clean) {
      AECM_TRY(b->s_clean.reserve(bytes));
      AECM_TRY(hipMemcpyAsync(b->s_clean.p, clean, bytes, hipMemcpyHostToDevice, b->stream));
      d_clean = (const int16_t*)b->s_clean.p;
    }
  }
  const int16_t* d_ms = nullptr;
  if (near) {
    AECM_TRY(b->s_ms.reserve(frames * sizeof(int16_t)));
    AECM_TRY(hipMemcpyAsync(b->s_ms.p, b->ms_host.data(), frames * sizeof(int16_t), hipMemcpyHostToDevice, b->stream));
    d_ms = (const int16_t*)b->s_ms.p;
  }
  AECM_TRY(launch_frames(b->state, b->work, b->tables, S, F, n, d_far, d_near, d_clean, d_out, d_ms, b->stream));
  if (mem == ASP_MEM_HOST && near)
    AECM_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, b->stream));
  // the clamped delays are staged from host memory that the next call rewrites
  AECM_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}
}  // namespace

extern "C" {

size_t AspAecm_state_size(void) { return sizeof(AspAecmState); }

int AspAecmBatch_Create(AspAecmBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return ASP_ERR_PARAM;
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_aecm", device, ASP_ERR_NO_DEVICE, "AspAecmBatch_Create: no HIP device")) return rc;
  AspAecmBatch* b = new AspAecmBatch;
  b->S = num_streams;
  b->device = device;
  b->inited.assign(num_streams, 0);
  b->last_error.assign(num_streams, 0);
  b->cng.assign(num_streams, 1);
  b->echo.assign(num_streams, 3);
  AecmTables T;
  build_tables(&T);
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, sizeof(AspAecmState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMalloc((void**)&b->work, sizeof(AecmWork) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMalloc((void**)&b->tables, sizeof(AecmTables));
  if (e == hipSuccess) e = hipMemset(b->state, 0, sizeof(AspAecmState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMemcpy(b->tables, &T, sizeof T, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    AspAecmBatch_Free(b);
    return aecm_fail(ASP_ERR_HIP, "AspAecmBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspAecmBatch_Free(AspAecmBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  void* bufs[] = {b->state, b->work, b->tables, b->s_far.p, b->s_near.p, b->s_clean.p, b->s_out.p, b->s_ms.p, b->s_path.p};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspAecmBatch_num_streams(const AspAecmBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspAecmBatch_InitStream(AspAecmBatch* b, int stream, int32_t sampFreq) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  if (sampFreq != 8000 && sampFreq != 16000) {
    b->last_error[stream] = AECM_BAD_PARAMETER_ERROR;
    return ASP_ERR_PARAM;
  }
  int r = control(b, stream, 1, 0, sampFreq, nullptr);
  if (r) return r;
  b->inited[stream] = 1;
  b->cng[stream] = 1;
  b->echo[stream] = 3;
  return ASP_OK;
}

int AspAecmBatch_Init(AspAecmBatch* b, int32_t sampFreq) {
  if (!b) return ASP_ERR_PARAM;
  if (sampFreq != 8000 && sampFreq != 16000) {
    for (int s = 0; s < b->S; ++s) b->last_error[s] = AECM_BAD_PARAMETER_ERROR;
    return ASP_ERR_PARAM;
  }
  int r = control(b, 0, b->S, 0, sampFreq, nullptr);
  if (r) return r;
  for (int s = 0; s < b->S; ++s) {
    b->inited[s] = 1;
    b->cng[s] = 1;
    b->echo[s] = 3;
  }
  return ASP_OK;
}

// WebRtcAecm_set_config: cngMode is stored before echoMode is checked, as in the reference
int AspAecmBatch_set_config_stream(AspAecmBatch* b, int stream, AecmConfig c) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  if (!b->inited[stream]) {
    b->last_error[stream] = AECM_UNINITIALIZED_ERROR;
    return ASP_ERR_PARAM;
  }
  if (c.cngMode != AecmFalse && c.cngMode != AecmTrue) {
    b->last_error[stream] = AECM_BAD_PARAMETER_ERROR;
    return ASP_ERR_PARAM;
  }
  if (c.echoMode < 0 || c.echoMode > 4) {
    // the reference has set cngMode already; keep the echo mode and its gains
    b->cng[stream] = c.cngMode;
    int r = control(b, stream, 1, 1, c.cngMode, nullptr);
    b->last_error[stream] = AECM_BAD_PARAMETER_ERROR;
    return r ? r : ASP_ERR_PARAM;
  }
  int r = control(b, stream, 1, 1, c.cngMode | ((c.echoMode + 1) << 1), nullptr);
  if (r) return r;
  b->cng[stream] = c.cngMode;
  b->echo[stream] = c.echoMode;
  return ASP_OK;
}

int AspAecmBatch_set_config(AspAecmBatch* b, AecmConfig c) {
  if (!b) return ASP_ERR_PARAM;
  for (int s = 0; s < b->S; ++s)
    if (!b->inited[s]) return aecm_fail(ASP_ERR_STATE, "AspAecmBatch_set_config: stream not initialised");
  if (c.cngMode != AecmFalse && c.cngMode != AecmTrue) return ASP_ERR_PARAM;
  if (c.echoMode < 0 || c.echoMode > 4) return ASP_ERR_PARAM;
  int r = control(b, 0, b->S, 1, c.cngMode | ((c.echoMode + 1) << 1), nullptr);
  if (r) return r;
  for (int s = 0; s < b->S; ++s) {
    b->cng[s] = c.cngMode;
    b->echo[s] = c.echoMode;
  }
  return ASP_OK;
}

int AspAecmBatch_InitEchoPath_stream(AspAecmBatch* b, int stream, const int16_t* path) {
  if (check_stream(b, stream) || !path) return ASP_ERR_PARAM;
  if (!b->inited[stream]) return ASP_ERR_STATE;
  return control(b, stream, 1, 2, 0, path);
}

int AspAecmBatch_GetEchoPath_stream(AspAecmBatch* b, int stream, int16_t* path) {
  if (check_stream(b, stream) || !path) return ASP_ERR_PARAM;
  if (!b->inited[stream]) return ASP_ERR_STATE;
  AspDeviceScope dev_scope_;
  AECM_TRY(dev_scope_.select(b->device));
  AECM_TRY(hipMemcpyAsync(path, &b->state[stream].channelStored[0], 65 * sizeof(int16_t), hipMemcpyDeviceToHost,
                          b->stream));
  AECM_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAecmBatch_BufferFarend(AspAecmBatch* b, const int16_t* far, int n, int mem) {
  if (!far) return ASP_ERR_PARAM;
  return run_frames(b, 1, far, nullptr, nullptr, nullptr, n, nullptr, nullptr, mem);
}

int AspAecmBatch_ProcessV(AspAecmBatch* b, const int16_t* near, const int16_t* clean, int16_t* out, int n,
                          const int16_t* ms, int mem) {
  if (!near || !out || !ms) return ASP_ERR_PARAM;
  return run_frames(b, 1, nullptr, near, clean, out, n, ms, nullptr, mem);
}

int AspAecmBatch_Process(AspAecmBatch* b, const int16_t* near, const int16_t* clean, int16_t* out, int n,
                         int16_t ms, int mem) {
  if (!b) return ASP_ERR_PARAM;
  std::vector<int16_t> v(b->S, ms);
  return AspAecmBatch_ProcessV(b, near, clean, out, n, v.data(), mem);
}

int AspAecmBatch_ProcessFrames(AspAecmBatch* b, int F, const int16_t* far, const int16_t* near, const int16_t* clean,
                               int16_t* out, int n, const int16_t* ms, int32_t* ret, int mem) {
  if (!near || !out || !ms) return ASP_ERR_PARAM;
  return run_frames(b, F, far, near, clean, out, n, ms, ret, mem);
}

int AspAecmBatch_get_error_code(AspAecmBatch* b, int stream) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  return b->last_error[stream];
}

int AspAecmBatch_ExportState(AspAecmBatch* b, int stream, AspAecmState* out) {
  if (check_stream(b, stream) || !out) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AECM_TRY(dev_scope_.select(b->device));
  AECM_TRY(hipMemcpyAsync(out, &b->state[stream], sizeof(AspAecmState), hipMemcpyDeviceToHost, b->stream));
  AECM_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAecmBatch_ImportState(AspAecmBatch* b, int stream, const AspAecmState* in) {
  if (check_stream(b, stream) || !in) return ASP_ERR_PARAM;
  if ((in->sampFreq != 8000 && in->sampFreq != 16000) || in->mult != in->sampFreq / 8000) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AECM_TRY(dev_scope_.select(b->device));
  AECM_TRY(hipMemcpyAsync(&b->state[stream], in, sizeof(AspAecmState), hipMemcpyHostToDevice, b->stream));
  AECM_TRY(hipStreamSynchronize(b->stream));
  b->inited[stream] = 1;
  b->cng[stream] = in->cngMode;
  b->echo[stream] = in->echoMode;
  return ASP_OK;
}

int AspAecmBatch_SetStream(AspAecmBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspAecmBatch_Synchronize(AspAecmBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AECM_TRY(dev_scope_.select(b->device));
  AECM_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

// ---------------------------------------------------------------- layer 1: a batch of one stream
int32_t WebRtcAecm_Create(void** inst) {
  if (!inst) return -1;
  AspAecmBatch* b = nullptr;
  if (AspAecmBatch_Create(&b, 1, 0) != ASP_OK) {
    *inst = nullptr;
    return -1;
  }
  *inst = b;
  return 0;
}

int32_t WebRtcAecm_Free(void* inst) {
  if (!inst) return -1;
  AspAecmBatch_Free((AspAecmBatch*)inst);
  return 0;
}

int32_t WebRtcAecm_Init(void* inst, int32_t sampFreq) {
  if (!inst) return -1;
  AspAecmBatch* b = (AspAecmBatch*)inst;
  return AspAecmBatch_InitStream(b, 0, sampFreq) == ASP_OK ? 0 : -1;
}

int32_t WebRtcAecm_BufferFarend(void* inst, const int16_t* farend, int16_t n) {
  if (!inst) return -1;
  AspAecmBatch* b = (AspAecmBatch*)inst;
  if (!farend) {
    b->last_error[0] = AECM_NULL_POINTER_ERROR;
    return -1;
  }
  if (!b->inited[0]) {
    b->last_error[0] = AECM_UNINITIALIZED_ERROR;
    return -1;
  }
  if (n != 80 && n != 160) {
    b->last_error[0] = AECM_BAD_PARAMETER_ERROR;
    return -1;
  }
  return run_frames(b, 1, farend, nullptr, nullptr, nullptr, n, nullptr, nullptr, ASP_MEM_HOST) == ASP_OK ? 0 : -1;
}

int32_t WebRtcAecm_Process(void* inst, const int16_t* nearN, const int16_t* nearC, int16_t* out, int16_t n,
                           int16_t ms) {
  if (!inst) return -1;
  AspAecmBatch* b = (AspAecmBatch*)inst;
  if (!nearN || !out) {
    b->last_error[0] = AECM_NULL_POINTER_ERROR;
    return -1;
  }
  if (!b->inited[0]) {
    b->last_error[0] = AECM_UNINITIALIZED_ERROR;
    return -1;
  }
  if (n != 80 && n != 160) {
    b->last_error[0] = AECM_BAD_PARAMETER_ERROR;
    return -1;
  }
  int32_t ret = 0;
  if (run_frames(b, 1, nullptr, nearN, nearC, out, n, &ms, &ret, ASP_MEM_HOST) != ASP_OK) return -1;
  return ret;
}

int32_t WebRtcAecm_set_config(void* inst, AecmConfig config) {
  if (!inst) return -1;
  return AspAecmBatch_set_config_stream((AspAecmBatch*)inst, 0, config) == ASP_OK ? 0 : -1;
}

int32_t WebRtcAecm_get_config(void* inst, AecmConfig* config) {
  if (!inst) return -1;
  AspAecmBatch* b = (AspAecmBatch*)inst;
  if (!config) {
    b->last_error[0] = AECM_NULL_POINTER_ERROR;
    return -1;
  }
  if (!b->inited[0]) {
    b->last_error[0] = AECM_UNINITIALIZED_ERROR;
    return -1;
  }
  config->cngMode = b->cng[0];
  config->echoMode = b->echo[0];
  return 0;
}

static int32_t echo_path_checks(AspAecmBatch* b, const void* p, size_t size_bytes) {
  if (!p) {
    b->last_error[0] = AECM_NULL_POINTER_ERROR;
    return -1;
  }
  if (size_bytes != WebRtcAecm_echo_path_size_bytes()) {
    b->last_error[0] = AECM_BAD_PARAMETER_ERROR;
    return -1;
  }
  if (!b->inited[0]) {
    b->last_error[0] = AECM_UNINITIALIZED_ERROR;
    return -1;
  }
  return 0;
}

int32_t WebRtcAecm_InitEchoPath(void* inst, const void* echo_path, size_t size_bytes) {
  if (!inst) return -1;
  AspAecmBatch* b = (AspAecmBatch*)inst;
  if (echo_path_checks(b, echo_path, size_bytes)) return -1;
  return AspAecmBatch_InitEchoPath_stream(b, 0, (const int16_t*)echo_path) == ASP_OK ? 0 : -1;
}

int32_t WebRtcAecm_GetEchoPath(void* inst, void* echo_path, size_t size_bytes) {
  if (!inst) return -1;
  AspAecmBatch* b = (AspAecmBatch*)inst;
  if (echo_path_checks(b, echo_path, size_bytes)) return -1;
  return AspAecmBatch_GetEchoPath_stream(b, 0, (int16_t*)echo_path) == ASP_OK ? 0 : -1;
}

size_t WebRtcAecm_echo_path_size_bytes(void) { return 65 * sizeof(int16_t); }

int32_t WebRtcAecm_get_error_code(void* inst) {
  if (!inst) return -1;
  return ((AspAecmBatch*)inst)->last_error[0];
}

}  // extern "C"
