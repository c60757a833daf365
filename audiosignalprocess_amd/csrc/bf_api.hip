// bf_api.hip -- host side of include/asp_bf.h: the batch handle (per stream an AspBfState and the buffer array
// in [M][384], out [384] in HBM), the Initialize-time tables (bf_core.h's make_tables on the host libm, uploaded
// once and shared by every stream), ProcessChunk's argument checks, staging for host-memory callers.  No CPU
// fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "api_common.h"
#include "bf_core.h"

namespace aspbf {
hipError_t launch_chunks(const BfParams& p, const BfTables& tb, AspBfState* states, float* bufs, int S, int F,
                         const float* input, const float* high, float* output, float* high_output, uint8_t* present,
                         hipStream_t stream);
}  // namespace aspbf

using namespace aspbf;

#define bf_fail(...) asp_fail("asp_bf", __VA_ARGS__)
#define BF_TRY(x) ASP_TRY("asp_bf", x)

struct AspBfBatch {
  int S = 0, device = 0;
  bool ready = false;
  BfParams p{};
  HostTables h;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspBfState* states = nullptr;  // [S]
  float* bufs = nullptr;         // [S][stride]
  size_t stride = 0;
  float* tables = nullptr;       // the kernel's table array (bf_layout.h)
  int tables_M = 0;
  AspStage s_in, s_high, s_out, s_high_out, s_present;  // staging for host-memory callers
};

namespace {
__global__ void bf_debug_hypotf_kernel(const float* x, const float* y, float* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = bf_hypotf(x[i], y[i]);
}

int upload_tables(AspBfBatch* b) {
  std::vector<float> pack;
  pack_tables(b->h, pack);
  BF_TRY(hipMemcpy(b->tables, pack.data(), sizeof(float) * pack.size(), hipMemcpyHostToDevice));
  return ASP_OK;
}

int init_streams(AspBfBatch* b, int first, int count) {
  AspBfState st;
  memset(&st, 0, sizeof st);
  init_state(st, b->p.M, b->p.hold);
  std::vector<AspBfState> all((size_t)count, st);
  BF_TRY(hipMemcpyAsync(b->states + first, all.data(), sizeof(AspBfState) * (size_t)count, hipMemcpyHostToDevice,
                        b->stream));
  BF_TRY(hipMemsetAsync(b->bufs + (size_t)first * b->stride, 0, sizeof(float) * b->stride * (size_t)count, b->stream));
  BF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int run(AspBfBatch* b, int F, const float* input, const float* high_input, float* output, float* high_output,
        uint8_t* target_present, int mem) {
  if (!b) return ASP_ERR_PARAM;
  if (!b->ready) return bf_fail(ASP_ERR_STATE, "AspBfBatch_ProcessChunk: not initialised");
  if ((mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE) || F < 0 || !input || !output)
    return bf_fail(ASP_ERR_PARAM, "AspBfBatch_ProcessChunk: NULL input or output, num_frames < 0 or a bad mem");
  if (high_input && !high_output)
    return bf_fail(ASP_ERR_PARAM, "AspBfBatch_ProcessChunk: high_input without high_output");
  if (F == 0) return ASP_OK;
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  const size_t U = (size_t)F * b->S;
  const size_t nb_in = U * b->p.M * kChunk * sizeof(float), nb_out = U * kChunk * sizeof(float);
  const float *d_in = input, *d_high = high_input;
  float *d_out = output, *d_high_out = high_input ? high_output : nullptr;
  uint8_t* d_present = target_present;
  if (mem == ASP_MEM_HOST) {
    BF_TRY(b->s_in.reserve(nb_in));
    BF_TRY(b->s_out.reserve(nb_out));
    BF_TRY(hipMemcpyAsync(b->s_in.p, input, nb_in, hipMemcpyHostToDevice, b->stream));
    d_in = (const float*)b->s_in.p;
    d_out = (float*)b->s_out.p;
    if (high_input) {
      BF_TRY(b->s_high.reserve(nb_in));
      BF_TRY(b->s_high_out.reserve(nb_out));
      BF_TRY(hipMemcpyAsync(b->s_high.p, high_input, nb_in, hipMemcpyHostToDevice, b->stream));
      d_high = (const float*)b->s_high.p;
      d_high_out = (float*)b->s_high_out.p;
    }
    if (target_present) {
      BF_TRY(b->s_present.reserve(U));
      d_present = (uint8_t*)b->s_present.p;
    }
  }
  BF_TRY(launch_chunks(b->p, view_tables(b->tables, b->p.M), b->states, b->bufs, b->S, F, d_in, d_high, d_out,
                       d_high_out, d_present, b->stream));
  if (mem == ASP_MEM_HOST) {
    BF_TRY(hipMemcpyAsync(output, d_out, nb_out, hipMemcpyDeviceToHost, b->stream));
    if (high_input) BF_TRY(hipMemcpyAsync(high_output, d_high_out, nb_out, hipMemcpyDeviceToHost, b->stream));
    if (target_present) BF_TRY(hipMemcpyAsync(target_present, d_present, U, hipMemcpyDeviceToHost, b->stream));
    BF_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}
}  // namespace

extern "C" {

size_t AspBf_state_size(void) { return sizeof(AspBfState); }

int AspBfBatch_Free(AspBfBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
  void* bufs[] = {b->states, b->bufs, b->tables, b->s_in.p, b->s_high.p, b->s_out.p, b->s_high_out.p, b->s_present.p};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspBfBatch_Create(AspBfBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return bf_fail(ASP_ERR_PARAM, "AspBfBatch_Create: NULL out or num_streams < 1");
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_bf", device, ASP_ERR_NO_DEVICE, "AspBfBatch_Create: no HIP device")) return rc;
  AspBfBatch* b = new AspBfBatch;
  b->S = num_streams;
  b->device = device;
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->states, sizeof(AspBfState) * (size_t)num_streams);
  if (e != hipSuccess) {
    AspBfBatch_Free(b);
    return bf_fail(ASP_ERR_HIP, "AspBfBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspBfBatch_num_streams(const AspBfBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspBfBatch_Initialize(AspBfBatch* b, int num_mics, const float* geometry_xyz, int chunk_size_ms,
                          int sample_rate_hz) {
  if (!b) return ASP_ERR_PARAM;
  HostTables h;
  BfParams p{};
  if (const char* why = make_tables(h, p, num_mics, geometry_xyz, chunk_size_ms, sample_rate_hz)) {
    char text[400];
    snprintf(text, sizeof text, "AspBfBatch_Initialize: %s", why);
    return bf_fail(ASP_ERR_PARAM, text);
  }
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  BF_TRY(hipStreamSynchronize(b->stream));
  const size_t stride = buffer_floats(p.M);
  if (stride != b->stride || !b->bufs || b->tables_M != p.M) {
    b->ready = false;
    if (b->bufs) (void)hipFree(b->bufs);
    if (b->tables) (void)hipFree(b->tables);
    b->bufs = b->tables = nullptr;
    BF_TRY(hipMalloc((void**)&b->bufs, sizeof(float) * stride * (size_t)b->S));
    BF_TRY(hipMalloc((void**)&b->tables, sizeof(float) * (size_t)pack_floats(p.M)));
    b->stride = stride;
    b->tables_M = p.M;
  }
  b->p = p;
  b->h = h;
  if (int rc = upload_tables(b)) return rc;
  if (int rc = init_streams(b, 0, b->S)) return rc;
  b->ready = true;
  return ASP_OK;
}

int AspBfBatch_InitializeStream(AspBfBatch* b, int stream) {
  if (!b || stream < 0 || stream >= b->S) return ASP_ERR_PARAM;
  if (!b->ready) return bf_fail(ASP_ERR_STATE, "AspBfBatch_InitializeStream: not initialised");
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  return init_streams(b, stream, 1);
}

int AspBfBatch_ProcessChunk(AspBfBatch* b, const float* input, const float* high_input, float* output,
                            float* high_output, uint8_t* target_present, int mem) {
  return run(b, 1, input, high_input, output, high_output, target_present, mem);
}

int AspBfBatch_ProcessChunks(AspBfBatch* b, int num_frames, const float* input, const float* high_input,
                             float* output, float* high_output, uint8_t* target_present, int mem) {
  return run(b, num_frames, input, high_input, output, high_output, target_present, mem);
}

int AspBfBatch_state_floats(const AspBfBatch* b) { return b && b->ready ? (int)b->stride : -1; }

int AspBfBatch_GetState(AspBfBatch* b, int stream, AspBfState* state, float* buffers) {
  if (!b || stream < 0 || stream >= b->S || !state || !buffers) return ASP_ERR_PARAM;
  if (!b->ready) return bf_fail(ASP_ERR_STATE, "AspBfBatch_GetState: not initialised");
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  BF_TRY(hipMemcpyAsync(state, b->states + stream, sizeof(AspBfState), hipMemcpyDeviceToHost, b->stream));
  BF_TRY(hipMemcpyAsync(buffers, b->bufs + (size_t)stream * b->stride, sizeof(float) * b->stride, hipMemcpyDeviceToHost,
                        b->stream));
  BF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspBfBatch_SetState(AspBfBatch* b, int stream, const AspBfState* state, const float* buffers) {
  if (!b || stream < 0 || stream >= b->S || !state || !buffers) return ASP_ERR_PARAM;
  if (!b->ready) return bf_fail(ASP_ERR_STATE, "AspBfBatch_SetState: not initialised");
  // the kernel indexes its buffers and mask rows with these: only the values the Blocker and the beamformer reach
  if (state->num_mics != b->p.M || state->frame_offset < 0 || state->frame_offset > 96 || state->frame_offset % 32 ||
      state->current_block_ix < 0 || state->current_block_ix > 1 || state->previous_block_ix < -1 ||
      state->previous_block_ix > 1)
    return bf_fail(ASP_ERR_PARAM, "AspBfBatch_SetState: the state's microphone count, frame offset or block indices are "
                                  "not ones this batch can reach");
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  BF_TRY(hipMemcpyAsync(b->states + stream, state, sizeof(AspBfState), hipMemcpyHostToDevice, b->stream));
  BF_TRY(hipMemcpyAsync(b->bufs + (size_t)stream * b->stride, buffers, sizeof(float) * b->stride, hipMemcpyHostToDevice,
                        b->stream));
  BF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspBfBatch_GetTables(AspBfBatch* b, int which, float* out, int cap) {
  if (!b || !out || which < 0 || which >= kTabCount) return ASP_ERR_PARAM;
  if (!b->ready) return bf_fail(ASP_ERR_STATE, "AspBfBatch_GetTables: not initialised");
  const std::vector<float>& t = b->h.t[which];
  if (cap < (int)t.size()) return bf_fail(ASP_ERR_PARAM, "AspBfBatch_GetTables: cap is below the table's length");
  memcpy(out, t.data(), sizeof(float) * t.size());
  return (int)t.size();
}

int AspBfBatch_SetTables(AspBfBatch* b, int which, const float* in, int count) {
  if (!b || !in || which < 0 || which >= kTabCount) return ASP_ERR_PARAM;
  if (!b->ready) return bf_fail(ASP_ERR_STATE, "AspBfBatch_SetTables: not initialised");
  if (count != table_length(which, b->p.M))
    return bf_fail(ASP_ERR_PARAM, "AspBfBatch_SetTables: count is not the table's length");
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  BF_TRY(hipStreamSynchronize(b->stream));
  b->h.t[which].assign(in, in + count);
  if (which == kTabDecay) b->p.decay = in[0];
  return upload_tables(b);
}

int AspBfBatch_SetStream(AspBfBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspBfBatch_Synchronize(AspBfBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  BF_TRY(dev_scope_.select(b->device));
  BF_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

// Test seam for the device math: out[i] = bf_hypotf(x[i], y[i]) evaluated on the device.
int AspBf_debug_hypotf(const float* x, const float* y, float* out, size_t n, int device) {
  if (!x || !y || !out || n == 0 || n > ((size_t)1 << 30)) return bf_fail(ASP_ERR_PARAM, "AspBf_debug_hypotf: bad argument");
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_bf", device, ASP_ERR_NO_DEVICE, "AspBf_debug_hypotf: no HIP device")) return rc;
  float* d = nullptr;  // x [n], y [n], out [n]
  BF_TRY(hipMalloc((void**)&d, 3 * n * sizeof(float)));
  hipError_t e = hipMemcpy(d, x, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, y, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(bf_debug_hypotf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, d, d + n, d + 2 * n, n);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return bf_fail(ASP_ERR_HIP, "AspBf_debug_hypotf", e);
  return ASP_OK;
}

}  // extern "C"
