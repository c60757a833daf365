// splrs_api.hip -- host side of include/asp_resampler.h: the batch handle (96 state words per channel of
// every stream in HBM), Resampler::Reset's mode table and Push's per-mode checks, staging for host-memory
// callers.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "api_common.h"
#include "splrs_core.h"

namespace aspsplrs {
hipError_t launch_push(int32_t* state, const int16_t* in, int16_t* out, int U, int ch, int mode, int len, int olen,
                       int F, hipStream_t stream);
}  // namespace aspsplrs

using namespace aspsplrs;

#define rs_fail(...) asp_fail("asp_resampler", __VA_ARGS__)
#define RS_TRY(x) ASP_TRY("asp_resampler", x)

struct AspResamplerBatch {
  int S = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  int32_t* state = nullptr;  // [S * 2][96]: room for two channels
  int mode = -1;             // -1: kResamplerInvalid
  int in_khz = 0, out_khz = 0, channels = 0;
  AspStage s_in, s_out;      // staging for host-memory callers
};

namespace {
int check_unit(AspResamplerBatch* b, int s, int c) {
  return (b && s >= 0 && s < b->S && c >= 0 && c < (b->channels ? b->channels : 1)) ? ASP_OK : ASP_ERR_PARAM;
}

// per-stream outLen for length_in interleaved samples, or -1
int out_length(const AspResamplerBatch* b, int length_in, int max_len) {
  if (!b || b->mode < 0) return -1;
  if (b->channels == 2) {
    if (length_in & 1) return -1;
    const int o = check_push(b->mode, length_in / 2, max_len / 2);
    return o < 0 ? -1 : 2 * o;
  }
  return check_push(b->mode, length_in, max_len);
}

int run(AspResamplerBatch* b, const int16_t* in, int len, int F, int16_t* out, int olen, int mem) {
  if (len == 0 || F == 0) return ASP_OK;
  const size_t ib = (size_t)F * b->S * len * sizeof(int16_t), ob = (size_t)F * b->S * olen * sizeof(int16_t);
  const char *i0 = (const char*)in, *o0 = (const char*)out;
  if (i0 < o0 + ob && o0 < i0 + ib) return rs_fail(ASP_ERR_PARAM, "AspResamplerBatch: in and out overlap");
  AspDeviceScope dev_scope_;
  RS_TRY(dev_scope_.select(b->device));
  const int16_t* d_in = in;
  int16_t* d_out = out;
  if (mem == ASP_MEM_HOST) {
    RS_TRY(b->s_in.reserve(ib));
    RS_TRY(b->s_out.reserve(ob ? ob : 2));
    RS_TRY(hipMemcpyAsync(b->s_in.p, in, ib, hipMemcpyHostToDevice, b->stream));
    d_in = (const int16_t*)b->s_in.p;
    d_out = (int16_t*)b->s_out.p;
  }
  const int ch = b->channels;
  RS_TRY(launch_push(b->state, d_in, d_out, b->S * ch, ch, b->mode, len / ch, olen / ch, F, b->stream));
  if (mem == ASP_MEM_HOST && ob) RS_TRY(hipMemcpyAsync(out, d_out, ob, hipMemcpyDeviceToHost, b->stream));
  RS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}
}  // namespace

extern "C" {

size_t AspResampler_state_size(void) { return sizeof(AspResamplerState); }

int AspResamplerBatch_Free(AspResamplerBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
  void* bufs[] = {b->state, b->s_in.p, b->s_out.p};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspResamplerBatch_Create(AspResamplerBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return rs_fail(ASP_ERR_PARAM, "AspResamplerBatch_Create: NULL out or num_streams < 1");
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_resampler", device, ASP_ERR_NO_DEVICE, "AspResamplerBatch_Create: no HIP device"))
    return rc;
  AspResamplerBatch* b = new AspResamplerBatch;
  b->S = num_streams;
  b->device = device;
  const size_t bytes = sizeof(int32_t) * kStateWords * 2 * (size_t)num_streams;
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, bytes);
  if (e == hipSuccess) e = hipMemset(b->state, 0, bytes);
  if (e != hipSuccess) {
    AspResamplerBatch_Free(b);
    return rs_fail(ASP_ERR_HIP, "AspResamplerBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspResamplerBatch_num_streams(const AspResamplerBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspResamplerBatch_Reset(AspResamplerBatch* b, int in_freq, int out_freq, int channels) {
  if (!b) return ASP_ERR_PARAM;
  b->mode = -1;
  if (channels != 1 && channels != 2) return -1;
  b->in_khz = in_freq / 1000;
  b->out_khz = out_freq / 1000;
  b->channels = channels;
  const int mode = select_mode(in_freq, out_freq);
  if (mode < 0) return -1;
  AspDeviceScope dev_scope_;
  RS_TRY(dev_scope_.select(b->device));
  // every Reset* of the reference zeroes its struct
  RS_TRY(hipMemsetAsync(b->state, 0, sizeof(int32_t) * kStateWords * 2 * (size_t)b->S, b->stream));
  RS_TRY(hipStreamSynchronize(b->stream));
  b->mode = mode;
  return 0;
}

int AspResamplerBatch_ResetIfNeeded(AspResamplerBatch* b, int in_freq, int out_freq, int channels) {
  if (!b) return ASP_ERR_PARAM;
  if (b->mode < 0 || in_freq / 1000 != b->in_khz || out_freq / 1000 != b->out_khz || channels != b->channels)
    return AspResamplerBatch_Reset(b, in_freq, out_freq, channels);
  return 0;
}

int AspResamplerBatch_ResetStream(AspResamplerBatch* b, int stream) {
  if (check_unit(b, stream, 0)) return ASP_ERR_PARAM;
  if (b->mode < 0) return -1;
  AspDeviceScope dev_scope_;
  RS_TRY(dev_scope_.select(b->device));
  const size_t row = sizeof(int32_t) * kStateWords * (size_t)b->channels;
  RS_TRY(hipMemsetAsync((char*)b->state + row * stream, 0, row, b->stream));
  RS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspResamplerBatch_OutLength(const AspResamplerBatch* b, int length_in) { return out_length(b, length_in, INT32_MAX); }

int AspResamplerBatch_Push(AspResamplerBatch* b, const int16_t* in, int length_in, int16_t* out, int max_len,
                           int* out_len, int mem) {
  if (!b || !in || !out || !out_len || (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE)) return ASP_ERR_PARAM;
  const int olen = out_length(b, length_in, max_len);
  if (olen < 0) return -1;
  if (int rc = run(b, in, length_in, 1, out, olen, mem)) return rc;
  *out_len = olen;
  return 0;
}

int AspResamplerBatch_PushFrames(AspResamplerBatch* b, const int16_t* in, int length_in, int num_frames, int16_t* out,
                                 int mem) {
  if (!b || !in || !out || num_frames < 0 || (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE)) return ASP_ERR_PARAM;
  const int olen = out_length(b, length_in, INT32_MAX);
  if (olen < 0) return -1;
  return run(b, in, length_in, num_frames, out, olen, mem);
}

int AspResamplerBatch_ExportState(AspResamplerBatch* b, int stream, int channel, AspResamplerState* out) {
  if (check_unit(b, stream, channel) || !out) return ASP_ERR_PARAM;
  if (b->mode < 0) return rs_fail(ASP_ERR_STATE, "AspResamplerBatch_ExportState: no valid Reset");
  AspDeviceScope dev_scope_;
  RS_TRY(dev_scope_.select(b->device));
  const int32_t* src = b->state + ((size_t)stream * b->channels + channel) * kStateWords;
  RS_TRY(hipMemcpyAsync(out->stage, src, sizeof out->stage, hipMemcpyDeviceToHost, b->stream));
  RS_TRY(hipStreamSynchronize(b->stream));
  out->mode = b->mode;
  out->in_freq_khz = b->in_khz;
  out->out_freq_khz = b->out_khz;
  return ASP_OK;
}

int AspResamplerBatch_ImportState(AspResamplerBatch* b, int stream, int channel, const AspResamplerState* in) {
  if (check_unit(b, stream, channel) || !in) return ASP_ERR_PARAM;
  if (b->mode < 0 || in->mode != b->mode)
    return rs_fail(ASP_ERR_PARAM, "AspResamplerBatch_ImportState: the state's mode is not the batch's");
  AspDeviceScope dev_scope_;
  RS_TRY(dev_scope_.select(b->device));
  int32_t* dst = b->state + ((size_t)stream * b->channels + channel) * kStateWords;
  RS_TRY(hipMemcpyAsync(dst, in->stage, sizeof in->stage, hipMemcpyHostToDevice, b->stream));
  RS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspResamplerBatch_SetStream(AspResamplerBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspResamplerBatch_Synchronize(AspResamplerBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  RS_TRY(dev_scope_.select(b->device));
  RS_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

}  // extern "C"
