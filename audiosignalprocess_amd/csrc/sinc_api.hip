// sinc_api.hip -- host side of include/asp_resample.h: kernel table, the position arithmetic of
// SincResampler::Resample / PushSincResampler::Resample run once per call for the whole batch
// (doubles, exactly the reference's recurrence), and the batch handle.  No CPU fallback.
#include <hip/hip_runtime.h>

#include "api_common.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "asp_ns.h"
#include "asp_resample.h"
#include "sinc_layout.h"
#include "sinc_plan.h"

using namespace aspsinc;

namespace aspsinc {
hipError_t launch_sinc(float* state, const float* kernel_table, const OutDesc* desc,
                       const int16_t* in, int16_t* out, int num_channels, int buf_len,
                       int src_frames, int dst_frames, const SincPlan& plan, hipStream_t s);
}

#define sinc_fail(...) asp_fail("asp_resample", __VA_ARGS__)
#define SINC_TRY(x) ASP_TRY("asp_resample", x)

struct AspSincBatch {
  int C = 0, device = 0, src = 0, dst = 0, buf_len = 0;
  hipStream_t stream = nullptr, own_stream = nullptr;
  float* state = nullptr;   // [C][buf_len]
  float* ktable = nullptr;  // [33 * 32]
  // descriptor tables: a ring of kDescRing slots on the device, each with a pinned host twin and the
  // event of the last kernel that read it (a call whose table differs from the previous one takes
  // the next slot: no stream synchronisation on the way)
  static constexpr int kDescRing = 4;
  OutDesc* desc = nullptr;         // [kDescRing][max_out]
  OutDesc* desc_pinned = nullptr;  // [kDescRing][max_out], hipHostMalloc
  hipEvent_t desc_ev[kDescRing] = {};
  size_t max_out = 0;
  int desc_slot = 0;
  int16_t *s_in = nullptr, *s_out = nullptr;
  std::vector<float> kernel_host;
  std::vector<OutDesc> desc_dev;  // the descriptor table as last uploaded
  std::vector<OutDesc> desc_host;
  // SincResampler / PushSincResampler position state (identical for every channel)
  double ratio = 0, vsi = 0;
  int r0 = 0, r3 = 0, r4 = 0, block_size = 0;
  bool primed = false, first_pass = true;
};

extern "C" {

int AspSincBatch_Create(AspSincBatch** out, int num_channels, int source_frames,
                        int destination_frames, int device) {
  AspDeviceScope dev_scope_;
  if (!out || num_channels <= 0 || source_frames <= kKernelSize || destination_frames <= 0)
    return sinc_fail(ASP_ERR_PARAM, "AspSincBatch_Create: bad argument");
  *out = nullptr;
  if (int rc = dev_scope_.select("asp_resample", device, ASP_ERR_PARAM, "no HIP device: the resampler has no CPU fallback")) return rc;
  AspSincBatch* b = new AspSincBatch();
  b->C = num_channels;
  b->device = device;
  b->src = source_frames;
  b->dst = destination_frames;
  b->buf_len = source_frames + kKernelSize;
  b->ratio = source_frames * 1.0 / destination_frames;  // push_sinc_resampler.cc:19
  b->vsi = 0;                                            // Flush, sinc_resampler.cc:335-341
  update_regions(b, false);
  init_kernel(b);
  const size_t max_out = (size_t)destination_frames * 2 + 64;
  b->max_out = max_out;
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  b->stream = b->own_stream;
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, (size_t)num_channels * b->buf_len * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->ktable, b->kernel_host.size() * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&b->desc, AspSincBatch::kDescRing * max_out * sizeof(OutDesc));
  if (e == hipSuccess) e = hipHostMalloc((void**)&b->desc_pinned, AspSincBatch::kDescRing * max_out * sizeof(OutDesc));
  for (int i = 0; i < AspSincBatch::kDescRing && e == hipSuccess; ++i)
    e = hipEventCreateWithFlags(&b->desc_ev[i], hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&b->s_in, (size_t)num_channels * source_frames * sizeof(int16_t));
  if (e == hipSuccess) e = hipMalloc((void**)&b->s_out, (size_t)num_channels * destination_frames * sizeof(int16_t));
  if (e == hipSuccess) e = hipMemsetAsync(b->state, 0, (size_t)num_channels * b->buf_len * sizeof(float), b->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(b->ktable, b->kernel_host.data(), b->kernel_host.size() * sizeof(float),
                       hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  if (e != hipSuccess) {
    AspSincBatch_Free(b);
    return sinc_fail(ASP_ERR_HIP, "AspSincBatch_Create", e);
  }
  *out = b;
  return ASP_OK;
}

int AspSincBatch_Free(AspSincBatch* b) {
  AspDeviceScope dev_scope_;
  if (!b) return -1;
  (void)dev_scope_.select(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  if (b->state) (void)hipFree(b->state);
  if (b->ktable) (void)hipFree(b->ktable);
  if (b->desc) (void)hipFree(b->desc);
  if (b->desc_pinned) (void)hipHostFree(b->desc_pinned);
  for (int i = 0; i < AspSincBatch::kDescRing; ++i)
    if (b->desc_ev[i]) (void)hipEventDestroy(b->desc_ev[i]);
  if (b->s_in) (void)hipFree(b->s_in);
  if (b->s_out) (void)hipFree(b->s_out);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return 0;
}

int AspSincBatch_SetStream(AspSincBatch* b, void* hip_stream) {
  AspDeviceScope dev_scope_;
  if (!b) return sinc_fail(ASP_ERR_PARAM, "null batch handle");
  SINC_TRY(dev_scope_.select(b->device));
  SINC_TRY(hipStreamSynchronize(b->stream));
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspSincBatch_num_channels(const AspSincBatch* b) { return b ? b->C : 0; }

int AspSincBatch_Resample(AspSincBatch* b, const int16_t* in, int16_t* out, int mem) {
  AspDeviceScope dev_scope_;
  if (!b || !in || !out) return sinc_fail(ASP_ERR_PARAM, "AspSincBatch_Resample: bad argument");
  SINC_TRY(dev_scope_.select(b->device));
  // PushSincResampler::Resample (push_sinc_resampler.cc:47-60): a priming pass on the first call
  SincPlan plan;
  memset(&plan, 0, sizeof plan);
  if (!plan_push(b, &plan)) return sinc_fail(ASP_ERR_STATE, "resampler plan: too many segments");
  const int16_t* din = in;
  int16_t* dout = out;
  if (mem == ASP_MEM_HOST) {
    SINC_TRY(hipMemcpyAsync(b->s_in, in, (size_t)b->C * b->src * sizeof(int16_t), hipMemcpyHostToDevice, b->stream));
    din = b->s_in;
    dout = b->s_out;
  } else if (mem != ASP_MEM_DEVICE) {
    return sinc_fail(ASP_ERR_PARAM, "mem must be ASP_MEM_HOST or ASP_MEM_DEVICE");
  }
  // The descriptor table repeats from call to call while the fractional position does: upload it only
  // when it differs from the one last uploaded, into the next slot of the ring (the kernel that read
  // that slot kDescRing uploads ago has long finished; its event says so without draining the stream).
  if (b->desc_host.size() > b->max_out) return sinc_fail(ASP_ERR_STATE, "descriptor table overflow");
  if (b->desc_dev.size() != b->desc_host.size() ||
      memcmp(b->desc_dev.data(), b->desc_host.data(), b->desc_host.size() * sizeof(OutDesc)) != 0) {
    b->desc_slot = (b->desc_slot + 1) % AspSincBatch::kDescRing;
    SINC_TRY(hipEventSynchronize(b->desc_ev[b->desc_slot]));
    OutDesc* pin = b->desc_pinned + (size_t)b->desc_slot * b->max_out;
    memcpy(pin, b->desc_host.data(), b->desc_host.size() * sizeof(OutDesc));
    SINC_TRY(hipMemcpyAsync(b->desc + (size_t)b->desc_slot * b->max_out, pin, b->desc_host.size() * sizeof(OutDesc),
                            hipMemcpyHostToDevice, b->stream));
    b->desc_dev = b->desc_host;
  }
  SINC_TRY(launch_sinc(b->state, b->ktable, b->desc + (size_t)b->desc_slot * b->max_out, din, dout, b->C, b->buf_len,
                       b->src, b->dst, plan, b->stream));
  SINC_TRY(hipEventRecord(b->desc_ev[b->desc_slot], b->stream));
  if (mem == ASP_MEM_HOST) {
    SINC_TRY(hipMemcpyAsync(out, dout, (size_t)b->C * b->dst * sizeof(int16_t), hipMemcpyDeviceToHost, b->stream));
    SINC_TRY(hipStreamSynchronize(b->stream));
  }
  return ASP_OK;
}

int AspSincBatch_Synchronize(AspSincBatch* b) {
  AspDeviceScope dev_scope_;
  if (!b) return sinc_fail(ASP_ERR_PARAM, "null batch handle");
  SINC_TRY(dev_scope_.select(b->device));
  SINC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

static_assert(sizeof(AspSincPos) == sizeof(SincPos), "AspSincPos is SincPos");

int AspSincBatch_ExportState(AspSincBatch* b, int channel, float* buffer, AspSincPos* pos) {
  AspDeviceScope dev_scope_;
  if (!b || channel < 0 || channel >= b->C || !buffer || !pos) return sinc_fail(ASP_ERR_PARAM, "ExportState: bad argument");
  SINC_TRY(dev_scope_.select(b->device));
  SINC_TRY(hipMemcpyAsync(buffer, b->state + (size_t)channel * b->buf_len, b->buf_len * sizeof(float), hipMemcpyDeviceToHost,
                          b->stream));
  SINC_TRY(hipStreamSynchronize(b->stream));
  const SincPos p = get_pos(b);
  memcpy(pos, &p, sizeof p);
  return ASP_OK;
}

int AspSincBatch_ImportState(AspSincBatch* b, int channel, const float* buffer, const AspSincPos* pos) {
  AspDeviceScope dev_scope_;
  if (!b || channel < 0 || channel >= b->C || !buffer || !pos) return sinc_fail(ASP_ERR_PARAM, "ImportState: bad argument");
  SincPos p;
  memcpy(&p, pos, sizeof p);
  if (!same_pos(p, get_pos(b)))
    return sinc_fail(ASP_ERR_STATE, "AspSincBatch_ImportState: the position record differs from the batch's");
  SINC_TRY(dev_scope_.select(b->device));
  SINC_TRY(hipMemcpyAsync(b->state + (size_t)channel * b->buf_len, buffer, b->buf_len * sizeof(float), hipMemcpyHostToDevice,
                          b->stream));
  SINC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspSincBatch_buffer_length(const AspSincBatch* b) { return b ? b->buf_len : 0; }

int AspSincBatch_kernel_table(const AspSincBatch* b, float* out, int capacity) {
  AspDeviceScope dev_scope_;
  if (!b || !out || capacity < (int)b->kernel_host.size()) return sinc_fail(ASP_ERR_PARAM, "kernel_table: bad argument");
  memcpy(out, b->kernel_host.data(), b->kernel_host.size() * sizeof(float));
  return (int)b->kernel_host.size();
}

}  // extern "C"
