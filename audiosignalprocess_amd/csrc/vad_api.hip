// vad_api.hip -- host side of include/asp_vad.h: the batch handle (every stream's AspVadState in HBM), the
// per-call validation of webrtc_vad.c, and the reference's WebRtcVad_* as a batch of one stream.
// No CPU fallback.
#include <hip/hip_runtime.h>

#include "api_common.h"

#include <stdio.h>
#include <string.h>

#include <vector>

#include "vad_layout.h"

namespace aspvad {
hipError_t launch_process(AspVadState* state, const int16_t* in, int S, int fs, int L, int F, int8_t* dec,
                          int32_t* lev, int16_t* feat, hipStream_t st);
hipError_t launch_init(AspVadState* state, int first, int count, int init, int mode, hipStream_t st);
hipError_t launch_gaussian(const int16_t* in, const int16_t* mean, const int16_t* std_, int n, int32_t* p,
                           int16_t* delta, hipStream_t st);
}  // namespace aspvad

#define vad_fail(...) asp_fail("asp_vad", __VA_ARGS__)
#define VAD_TRY(x) ASP_TRY("asp_vad", x)

struct AspVadBatch {
  int S = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspVadState* state = nullptr;          // [S]
  std::vector<unsigned char> inited;     // host mirror of init_flag == 42, per stream
  AspStage s_in, s_dec, s_lev;           // staging for host-memory callers
};

extern "C" {

int WebRtcVad_ValidRateAndFrameLength(int rate, int frame_length) {
  if (rate != 8000 && rate != 16000 && rate != 32000 && rate != 48000) return -1;
  for (int ms = 10; ms <= 30; ms += 10)
    if (frame_length == rate / 1000 * ms) return 0;
  return -1;
}

int AspVadBatch_Create(AspVadBatch** out, int num_streams, int device) {
  AspDeviceScope dev_scope_;
  if (!out || num_streams <= 0) return vad_fail(ASP_ERR_PARAM, "AspVadBatch_Create: bad argument");
  *out = nullptr;
  if (int rc = dev_scope_.select("asp_vad", device, ASP_ERR_PARAM, "no HIP device: the VAD has no CPU fallback")) return rc;
  AspVadBatch* b = new AspVadBatch();
  b->S = num_streams;
  b->device = device;
  b->inited.assign(num_streams, 0);
  const size_t bytes = (size_t)num_streams * sizeof(AspVadState);
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  b->stream = b->own_stream;
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, bytes);
  if (e == hipSuccess) e = hipMemsetAsync(b->state, 0, bytes, b->stream);   // init_flag 0: uninitialised
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) {
    AspVadBatch_Free(b);
    return vad_fail(ASP_ERR_HIP, "AspVadBatch_Create", e);
  }
  *out = b;
  return ASP_OK;
}

int AspVadBatch_Free(AspVadBatch* b) {
  AspDeviceScope dev_scope_;
  if (!b) return ASP_ERR_PARAM;
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->state) (void)hipFree(b->state);
  b->s_in.release();
  b->s_dec.release();
  b->s_lev.release();
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspVadBatch_num_streams(const AspVadBatch* b) { return b ? b->S : 0; }

static int init_range(AspVadBatch* b, int first, int count, int init, int mode) {
  AspDeviceScope dev_scope_;
  VAD_TRY(dev_scope_.select(b->device));
  VAD_TRY(aspvad::launch_init(b->state, first, count, init, mode, b->stream));
  if (init) memset(b->inited.data() + first, 1, (size_t)count);
  return ASP_OK;
}

int AspVadBatch_Init(AspVadBatch* b) {
  if (!b) return vad_fail(ASP_ERR_PARAM, "null batch handle");
  return init_range(b, 0, b->S, 1, 0);
}

int AspVadBatch_InitStream(AspVadBatch* b, int stream) {
  if (!b || stream < 0 || stream >= b->S) return vad_fail(ASP_ERR_PARAM, "AspVadBatch_InitStream: bad argument");
  return init_range(b, stream, 1, 1, 0);
}

int AspVadBatch_set_mode(AspVadBatch* b, int mode) {
  if (!b || mode < 0 || mode > 3) return vad_fail(ASP_ERR_PARAM, "AspVadBatch_set_mode: bad argument");
  for (int s = 0; s < b->S; ++s)
    if (!b->inited[s]) return vad_fail(ASP_ERR_STATE, "AspVadBatch_set_mode: stream not initialised");
  return init_range(b, 0, b->S, 0, mode);
}

int AspVadBatch_set_mode_stream(AspVadBatch* b, int stream, int mode) {
  if (!b || stream < 0 || stream >= b->S || mode < 0 || mode > 3)
    return vad_fail(ASP_ERR_PARAM, "AspVadBatch_set_mode_stream: bad argument");
  if (!b->inited[stream]) return vad_fail(ASP_ERR_STATE, "AspVadBatch_set_mode_stream: stream not initialised");
  return init_range(b, stream, 1, 0, mode);
}

int AspVadBatch_Process(AspVadBatch* b, int fs, int frame_length, const int16_t* in, int num_frames,
                        int8_t* decisions, int32_t* levels, int mem) {
  AspDeviceScope dev_scope_;
  if (!b || !in || !decisions || num_frames <= 0) return vad_fail(ASP_ERR_PARAM, "AspVadBatch_Process: bad argument");
  if (WebRtcVad_ValidRateAndFrameLength(fs, frame_length) != 0)
    return vad_fail(ASP_ERR_PARAM, "AspVadBatch_Process: invalid rate / frame length");
  for (int s = 0; s < b->S; ++s)
    if (!b->inited[s]) return vad_fail(ASP_ERR_STATE, "AspVadBatch_Process: stream not initialised");
  VAD_TRY(dev_scope_.select(b->device));
  const size_t n = (size_t)num_frames * b->S;
  const size_t in_bytes = n * frame_length * sizeof(int16_t);
  const int16_t* din = in;
  int8_t* ddec = decisions;
  int32_t* dlev = levels;
  if (mem == ASP_MEM_HOST) {
    VAD_TRY(b->s_in.reserve(in_bytes));
    VAD_TRY(b->s_dec.reserve(n));
    if (levels) VAD_TRY(b->s_lev.reserve(n * sizeof(int32_t)));
    VAD_TRY(hipMemcpyAsync(b->s_in.p, in, in_bytes, hipMemcpyHostToDevice, b->stream));
    din = (const int16_t*)b->s_in.p;
    ddec = (int8_t*)b->s_dec.p;
    dlev = levels ? (int32_t*)b->s_lev.p : nullptr;
  } else if (mem != ASP_MEM_DEVICE) {
    return vad_fail(ASP_ERR_PARAM, "mem must be ASP_MEM_HOST or ASP_MEM_DEVICE");
  } else if (((uintptr_t)in & 3) != 0) {
    return vad_fail(ASP_ERR_PARAM, "AspVadBatch_Process: device input must be 4-byte aligned");
  }
  VAD_TRY(aspvad::launch_process(b->state, din, b->S, fs, frame_length, num_frames, ddec, dlev, nullptr, b->stream));
  if (mem == ASP_MEM_HOST) {
    VAD_TRY(hipMemcpyAsync(decisions, ddec, n, hipMemcpyDeviceToHost, b->stream));
    if (levels) VAD_TRY(hipMemcpyAsync(levels, dlev, n * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    VAD_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}

int AspVadBatch_Features(AspVadBatch* b, const int16_t* in, int frame_length, int16_t* features, int mem) {
  AspDeviceScope dev_scope_;
  if (!b || !in || !features || WebRtcVad_ValidRateAndFrameLength(8000, frame_length) != 0)
    return vad_fail(ASP_ERR_PARAM, "AspVadBatch_Features: bad argument");
  VAD_TRY(dev_scope_.select(b->device));
  const size_t in_bytes = (size_t)b->S * frame_length * sizeof(int16_t), out_bytes = (size_t)b->S * 7 * sizeof(int16_t);
  const int16_t* din = in;
  int16_t* dout = features;
  if (mem == ASP_MEM_HOST) {
    VAD_TRY(b->s_in.reserve(in_bytes));
    VAD_TRY(b->s_lev.reserve(out_bytes));
    VAD_TRY(hipMemcpyAsync(b->s_in.p, in, in_bytes, hipMemcpyHostToDevice, b->stream));
    din = (const int16_t*)b->s_in.p;
    dout = (int16_t*)b->s_lev.p;
  } else if (mem != ASP_MEM_DEVICE || ((uintptr_t)in & 3) != 0) {
    return vad_fail(ASP_ERR_PARAM, "AspVadBatch_Features: bad memory argument");
  }
  VAD_TRY(aspvad::launch_process(b->state, din, b->S, 8000, frame_length, 1, nullptr, nullptr, dout, b->stream));
  if (mem == ASP_MEM_HOST) {
    VAD_TRY(hipMemcpyAsync(features, dout, out_bytes, hipMemcpyDeviceToHost, b->stream));
    VAD_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}

int AspVadBatch_ExportState(AspVadBatch* b, int stream, AspVadState* out) {
  AspDeviceScope dev_scope_;
  if (!b || !out || stream < 0 || stream >= b->S) return vad_fail(ASP_ERR_PARAM, "ExportState: bad argument");
  VAD_TRY(dev_scope_.select(b->device));
  VAD_TRY(hipMemcpyAsync(out, b->state + stream, sizeof *out, hipMemcpyDeviceToHost, b->stream));
  VAD_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspVadBatch_ImportState(AspVadBatch* b, int stream, const AspVadState* in) {
  AspDeviceScope dev_scope_;
  if (!b || !in || stream < 0 || stream >= b->S) return vad_fail(ASP_ERR_PARAM, "ImportState: bad argument");
  VAD_TRY(dev_scope_.select(b->device));
  VAD_TRY(hipMemcpyAsync(b->state + stream, in, sizeof *in, hipMemcpyHostToDevice, b->stream));
  VAD_TRY(hipStreamSynchronize(b->stream));
  b->inited[stream] = in->init_flag == aspvad::kInitCheck;
  return ASP_OK;
}

int AspVadBatch_SetStream(AspVadBatch* b, void* hip_stream) {
  AspDeviceScope dev_scope_;
  if (!b) return vad_fail(ASP_ERR_PARAM, "null batch handle");
  VAD_TRY(dev_scope_.select(b->device));
  VAD_TRY(hipStreamSynchronize(b->stream));
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspVadBatch_Synchronize(AspVadBatch* b) {
  AspDeviceScope dev_scope_;
  if (!b) return vad_fail(ASP_ERR_PARAM, "null batch handle");
  VAD_TRY(dev_scope_.select(b->device));
  VAD_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspVad_debug_gaussian(const int16_t* input, const int16_t* mean, const int16_t* std_, int n,
                          int32_t* probability, int16_t* delta, int device) {
  AspDeviceScope dev_scope_;
  if (!input || !mean || !std_ || !probability || !delta || n <= 0)
    return vad_fail(ASP_ERR_PARAM, "AspVad_debug_gaussian: bad argument");
  if (int rc = dev_scope_.select("asp_vad", device, ASP_ERR_NO_DEVICE, "no HIP device")) return rc;
  int16_t* d = nullptr;
  const size_t b16 = (size_t)n * sizeof(int16_t);
  VAD_TRY(hipMalloc((void**)&d, 4 * b16 + (size_t)n * sizeof(int32_t)));
  int32_t* dp = (int32_t*)(d + 4 * (size_t)n);
  hipError_t e = hipMemcpy(d, input, b16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, mean, b16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 2 * (size_t)n, std_, b16, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = aspvad::launch_gaussian(d, d + n, d + 2 * (size_t)n, n, dp, d + 3 * (size_t)n, nullptr);
  if (e == hipSuccess) e = hipMemcpy(probability, dp, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(delta, d + 3 * (size_t)n, b16, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  return e == hipSuccess ? ASP_OK : vad_fail(ASP_ERR_HIP, "AspVad_debug_gaussian", e);
}

// ------------------------------------------------------------------ layer 1
struct WebRtcVadInst {
  AspVadBatch* b;
  int init_flag;
};

int WebRtcVad_Create(VadInst** handle) {
  if (!handle) return -1;
  *handle = nullptr;
  AspVadBatch* b = nullptr;
  if (AspVadBatch_Create(&b, 1, 0) != ASP_OK) return -1;
  *handle = new WebRtcVadInst{b, 0};
  return 0;
}

void WebRtcVad_Free(VadInst* handle) {
  if (!handle) return;
  AspVadBatch_Free(handle->b);
  delete handle;
}

int WebRtcVad_Init(VadInst* handle) {
  if (!handle || AspVadBatch_Init(handle->b) != ASP_OK) return -1;
  handle->init_flag = aspvad::kInitCheck;
  return 0;
}

int WebRtcVad_set_mode(VadInst* handle, int mode) {
  if (!handle || handle->init_flag != aspvad::kInitCheck || mode < 0 || mode > 3) return -1;
  return AspVadBatch_set_mode(handle->b, mode) == ASP_OK ? 0 : -1;
}

int WebRtcVad_Process(VadInst* handle, int fs, const int16_t* audio_frame, int frame_length) {
  if (!handle || handle->init_flag != aspvad::kInitCheck || !audio_frame) return -1;
  if (WebRtcVad_ValidRateAndFrameLength(fs, frame_length) != 0) return -1;
  int8_t d = 0;
  if (AspVadBatch_Process(handle->b, fs, frame_length, audio_frame, 1, &d, nullptr, ASP_MEM_HOST) != ASP_OK) return -1;
  return d;
}

}  // extern "C"
