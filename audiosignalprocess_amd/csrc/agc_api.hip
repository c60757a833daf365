// agc_api.hip -- host side of include/asp_agc.h: the batch handle (every stream's AspAgcState and stored
// microphone level in HBM), Init / set_config / get_config as host logic on a host copy of the stream's state
// (agc_core.h compiled for the host: the gain table is the code the kernel would run), the per-call
// validation, staging for host-memory callers, and the reference's WebRtcAgc_* as a batch of one stream.
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "api_common.h"
#include "agc_core.h"

namespace aspagc {
struct FrameArgs {
  AspAgcState* state;
  int32_t* level;
  int S, F, n, nb, ops;
  const int16_t *far, *low_in, *high_in;
  int16_t *low_out, *high_out;
  const int32_t* level_in;
  const int16_t* echo;
  int32_t *level_out, *vm_out;
  uint8_t* saturation;
  int32_t* rc;
};
hipError_t launch_frames(const FrameArgs& a, hipStream_t stream);
}  // namespace aspagc

using namespace aspagc;

#define agc_fail(...) asp_fail("asp_agc", __VA_ARGS__)
#define AGC_TRY(x) ASP_TRY("asp_agc", x)

struct AspAgcBatch {
  int S = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspAgcState* state = nullptr;  // [S]
  int32_t* level = nullptr;      // [S]
  std::vector<uint32_t> fs;      // per stream; 0: not initialised
  AspStage rc;                   // [F][S] return values of the last call
  size_t rc_count = 0;
  AspStage stage[10];            // staging for host-memory callers
  std::vector<AspAgcState> host; // scratch of Init / set_config
};

namespace {
bool valid_fs(uint32_t fs) { return fs == 8000 || fs == 16000 || fs == 32000 || fs == 48000; }
int check_stream(const AspAgcBatch* b, int s) { return (b && s >= 0 && s < b->S) ? ASP_OK : ASP_ERR_PARAM; }

// states [first, first + count) to the host scratch / back
int fetch(AspAgcBatch* b, int first, int count) {
  b->host.resize(count);
  AGC_TRY(hipMemcpyAsync(b->host.data(), b->state + first, sizeof(AspAgcState) * (size_t)count, hipMemcpyDeviceToHost, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}
int put(AspAgcBatch* b, int first, int count) {
  AGC_TRY(hipMemcpyAsync(b->state + first, b->host.data(), sizeof(AspAgcState) * (size_t)count, hipMemcpyHostToDevice, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int init_range(AspAgcBatch* b, int first, int count, int32_t lo, int32_t hi, int16_t mode, uint32_t fs) {
  if (!valid_fs(fs) || mode < 0 || mode > 3) return -1;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  if (int rc = fetch(b, first, count)) return rc;
  int ret = 0;
  std::vector<int32_t> lv(count);
  for (int i = 0; i < count; ++i) {
    ret = init_core(b->host[i], lo, hi, mode, fs);
    lv[i] = b->host[i].micVol;
  }
  if (int rc = put(b, first, count)) return rc;
  AGC_TRY(hipMemcpyAsync(b->level + first, lv.data(), sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  for (int i = 0; i < count; ++i) b->fs[first + i] = fs;
  return ret;
}

int config_range(AspAgcBatch* b, int first, int count, WebRtcAgcConfig c) {
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  if (int rc = fetch(b, first, count)) return rc;
  int ret = 0;
  for (int i = 0; i < count; ++i)
    if (set_config_core(b->host[i], c.targetLevelDbfs, c.compressionGaindB, c.limiterEnable) != 0) ret = -1;
  if (int rc = put(b, first, count)) return rc;
  return ret;
}

int set_level(AspAgcBatch* b, int first, int count, int32_t level) {
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  std::vector<int32_t> lv(count, level);
  AGC_TRY(hipMemcpyAsync(b->level + first, lv.data(), sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

struct Call {
  int F = 1, ops = 0, nb = 1, n = 0, mem = ASP_MEM_HOST;
  const int16_t *far = nullptr, *low_in = nullptr, *high_in = nullptr;
  int16_t *low_out = nullptr, *high_out = nullptr;
  const int32_t* level_in = nullptr;
  const int16_t* echo = nullptr;
  int32_t *level_out = nullptr, *vm_out = nullptr;
  uint8_t* saturation = nullptr;
};

int run(AspAgcBatch* b, const Call& c) {
  if (!b || c.F < 0 || (c.mem != ASP_MEM_HOST && c.mem != ASP_MEM_DEVICE)) return ASP_ERR_PARAM;
  if ((c.n != 80 && c.n != 160) || c.nb < 1 || c.nb > 3) return ASP_ERR_PARAM;
  const bool audio = (c.ops & ~kOpFar) != 0;
  if (audio && (!c.low_in || !c.low_out || (c.nb > 1 && (!c.high_in || !c.high_out)))) return ASP_ERR_PARAM;
  if ((c.ops & kOpFar) && !c.far) return ASP_ERR_PARAM;
  for (int s = 0; s < b->S; ++s) {
    if (!b->fs[s]) return agc_fail(ASP_ERR_STATE, "AspAgcBatch: stream not initialised");
    if ((b->fs[s] == 8000 ? 80 : 160) != c.n)
      return agc_fail(ASP_ERR_STATE, "AspAgcBatch: a stream was initialised for the other frame length");
  }
  if (c.F == 0) return ASP_OK;
  const size_t FS = (size_t)c.F * b->S, lb = FS * c.n * sizeof(int16_t), hb = lb * (c.nb - 1);
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  AGC_TRY(b->rc.reserve(FS * sizeof(int32_t)));
  b->rc_count = FS;
  FrameArgs a = {b->state, b->level, b->S, c.F, c.n, c.nb, c.ops, c.far, c.low_in, c.high_in, c.low_out, c.high_out,
                 c.level_in, c.echo, c.level_out, c.vm_out, c.saturation, (int32_t*)b->rc.p};
  struct Back {
    void* host;
    const void* dev;
    size_t bytes;
  } back[5];
  int nback = 0;
  if (c.mem == ASP_MEM_HOST) {
    int k = 0;
    auto in = [&](const void* p, size_t bytes, const void** d) -> hipError_t {
      AspStage& st = b->stage[k++];
      if (!p) return hipSuccess;
      hipError_t e = st.reserve(bytes);
      if (e == hipSuccess) e = hipMemcpyAsync(st.p, p, bytes, hipMemcpyHostToDevice, b->stream);
      *d = st.p;
      return e;
    };
    auto out = [&](void* p, size_t bytes, void** d) -> hipError_t {
      AspStage& st = b->stage[k++];
      if (!p) return hipSuccess;
      hipError_t e = st.reserve(bytes);
      *d = st.p;
      back[nback++] = {p, st.p, bytes};
      return e;
    };
    AGC_TRY(in(c.far, lb, (const void**)&a.far));
    AGC_TRY(in(c.low_in, lb, (const void**)&a.low_in));
    AGC_TRY(in(c.high_in, hb, (const void**)&a.high_in));
    AGC_TRY(in(c.level_in, FS * sizeof(int32_t), (const void**)&a.level_in));
    AGC_TRY(in(c.echo, FS * sizeof(int16_t), (const void**)&a.echo));
    AGC_TRY(out(c.low_out, lb, (void**)&a.low_out));
    AGC_TRY(out(c.nb > 1 ? c.high_out : nullptr, hb, (void**)&a.high_out));
    AGC_TRY(out(c.level_out, FS * sizeof(int32_t), (void**)&a.level_out));
    AGC_TRY(out(c.vm_out, FS * sizeof(int32_t), (void**)&a.vm_out));
    AGC_TRY(out(c.saturation, FS, (void**)&a.saturation));
  }
  AGC_TRY(launch_frames(a, b->stream));
  for (int i = 0; i < nback; ++i)
    AGC_TRY(hipMemcpyAsync(back[i].host, back[i].dev, back[i].bytes, hipMemcpyDeviceToHost, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int first_return(AspAgcBatch* b) {
  int32_t rc = -1;
  if (AspAgcBatch_returns(b, &rc, 1) != ASP_OK) return -1;
  return rc;
}

// layer 1: a stream's bands as the planes of a batch of one
struct Planes {
  int16_t hi[2 * 160];
  bool gather(const int16_t* const* in, int nb, int n) {
    if (!in) return false;
    for (int k = 0; k < nb; ++k)
      if (!in[k]) return false;
    for (int k = 1; k < nb; ++k) memcpy(hi + (k - 1) * n, in[k], n * sizeof(int16_t));
    return true;
  }
  void scatter(int16_t* const* out, int nb, int n) const {
    for (int k = 1; k < nb; ++k) memcpy(out[k], hi + (k - 1) * n, n * sizeof(int16_t));
  }
};
bool good_frame(const AspAgcBatch* b, int nb, int n) {
  return b && b->fs[0] && nb >= 1 && nb <= 3 && n == (b->fs[0] == 8000 ? 80 : 160);
}
}  // namespace

extern "C" {

size_t AspAgc_state_size(void) { return sizeof(AspAgcState); }
int AspAgc_gain_table(int32_t* table, int16_t comp, int16_t target, uint8_t limiter, int16_t analogTarget) {
  if (!table) return ASP_ERR_PARAM;
  return calculate_gain_table(table, comp, target, limiter, analogTarget);
}

int AspAgcBatch_Free(AspAgcBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
  if (b->state) (void)hipFree(b->state);
  if (b->level) (void)hipFree(b->level);
  b->rc.release();
  for (AspStage& s : b->stage) s.release();
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspAgcBatch_Create(AspAgcBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return agc_fail(ASP_ERR_PARAM, "AspAgcBatch_Create: NULL out or num_streams < 1");
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_agc", device, ASP_ERR_NO_DEVICE, "AspAgcBatch_Create: no HIP device")) return rc;
  AspAgcBatch* b = new AspAgcBatch;
  b->S = num_streams;
  b->device = device;
  b->fs.assign(num_streams, 0);
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, sizeof(AspAgcState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMalloc((void**)&b->level, sizeof(int32_t) * (size_t)num_streams);
  // on the batch's own (non-blocking) stream: a null-stream memset is not ordered with the copies Init puts on it
  if (e == hipSuccess) e = hipMemsetAsync(b->state, 0, sizeof(AspAgcState) * (size_t)num_streams, b->own_stream);
  if (e == hipSuccess) e = hipMemsetAsync(b->level, 0, sizeof(int32_t) * (size_t)num_streams, b->own_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->own_stream);
  if (e != hipSuccess) {
    AspAgcBatch_Free(b);
    return agc_fail(ASP_ERR_HIP, "AspAgcBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspAgcBatch_num_streams(const AspAgcBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspAgcBatch_Init(AspAgcBatch* b, int32_t lo, int32_t hi, int16_t mode, uint32_t fs) {
  if (!b) return ASP_ERR_PARAM;
  return init_range(b, 0, b->S, lo, hi, mode, fs);
}
int AspAgcBatch_InitStream(AspAgcBatch* b, int stream, int32_t lo, int32_t hi, int16_t mode, uint32_t fs) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  return init_range(b, stream, 1, lo, hi, mode, fs);
}
int AspAgcBatch_set_config(AspAgcBatch* b, WebRtcAgcConfig c) {
  if (!b) return ASP_ERR_PARAM;
  return config_range(b, 0, b->S, c);
}
int AspAgcBatch_set_config_stream(AspAgcBatch* b, int stream, WebRtcAgcConfig c) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  return config_range(b, stream, 1, c);
}
int AspAgcBatch_get_config_stream(AspAgcBatch* b, int stream, WebRtcAgcConfig* c) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  if (int rc = fetch(b, stream, 1)) return rc;
  AspAgcState& s = b->host[0];
  if (!c || s.initFlag != 42) {
    s.lastError = (int16_t)(!c ? AGC_NULL_POINTER_ERROR : AGC_UNINITIALIZED_ERROR);
    if (int rc = put(b, stream, 1)) return rc;
    return -1;
  }
  c->limiterEnable = s.usedConfig_limiterEnable;
  c->targetLevelDbfs = s.usedConfig_targetLevelDbfs;
  c->compressionGaindB = s.usedConfig_compressionGaindB;
  return 0;
}
int AspAgcBatch_last_error_stream(AspAgcBatch* b, int stream) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  if (int rc = fetch(b, stream, 1)) return rc;
  return (uint16_t)b->host[0].lastError;
}
int AspAgcBatch_set_mic_level(AspAgcBatch* b, int32_t level) {
  if (!b) return ASP_ERR_PARAM;
  return set_level(b, 0, b->S, level);
}
int AspAgcBatch_set_mic_level_stream(AspAgcBatch* b, int stream, int32_t level) {
  if (check_stream(b, stream)) return ASP_ERR_PARAM;
  return set_level(b, stream, 1, level);
}
int AspAgcBatch_get_mic_level_stream(AspAgcBatch* b, int stream, int32_t* level) {
  if (check_stream(b, stream) || !level) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  AGC_TRY(hipMemcpyAsync(level, b->level + stream, sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAgcBatch_AddFarend(AspAgcBatch* b, const int16_t* far, int samples, int mem) {
  Call c;
  c.ops = kOpFar;
  c.n = samples;
  c.far = far;
  c.mem = mem;
  return run(b, c);
}
int AspAgcBatch_AddMic(AspAgcBatch* b, int16_t* low, int16_t* high, int nb, int n, int mem) {
  Call c;
  c.ops = kOpAddMic;
  c.nb = nb;
  c.n = n;
  c.low_in = c.low_out = low;
  c.high_in = c.high_out = high;
  c.mem = mem;
  return run(b, c);
}
int AspAgcBatch_VirtualMic(AspAgcBatch* b, int16_t* low, int16_t* high, int nb, int n, const int32_t* level_in,
                           int32_t* level_out, int mem) {
  if (!level_in || !level_out) return ASP_ERR_PARAM;
  Call c;
  c.ops = kOpVirtualMic;
  c.nb = nb;
  c.n = n;
  c.low_in = c.low_out = low;
  c.high_in = c.high_out = high;
  c.level_in = level_in;
  c.vm_out = level_out;
  c.mem = mem;
  return run(b, c);
}
int AspAgcBatch_Process(AspAgcBatch* b, const int16_t* li, const int16_t* hi, int16_t* lo, int16_t* ho, int nb, int n,
                        const int32_t* level_in, const int16_t* echo, int32_t* level_out, uint8_t* saturation, int mem) {
  if (!level_in || !level_out || !saturation) return ASP_ERR_PARAM;
  Call c;
  c.ops = kOpProcess;
  c.nb = nb;
  c.n = n;
  c.low_in = li;
  c.high_in = hi;
  c.low_out = lo;
  c.high_out = ho;
  c.level_in = level_in;
  c.echo = echo;
  c.level_out = level_out;
  c.saturation = saturation;
  c.mem = mem;
  return run(b, c);
}
int AspAgcBatch_ProcessFrames(AspAgcBatch* b, int F, const int16_t* far, const int16_t* li, const int16_t* hi, int16_t* lo,
                              int16_t* ho, int nb, int n, const int32_t* level_in, const int16_t* echo, int32_t* level_out,
                              uint8_t* saturation, int mem) {
  Call c;
  c.F = F;
  c.ops = kOpByMode | kOpProcess | (far ? kOpFar : 0);
  c.nb = nb;
  c.n = n;
  c.far = far;
  c.low_in = li;
  c.high_in = hi;
  c.low_out = lo;
  c.high_out = ho;
  c.level_in = level_in;
  c.echo = echo;
  c.level_out = level_out;
  c.saturation = saturation;
  c.mem = mem;
  return run(b, c);
}

int AspAgcBatch_returns(AspAgcBatch* b, int32_t* out, int count) {
  if (!b || !out || count < 0 || (size_t)count > b->rc_count) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  AGC_TRY(hipMemcpyAsync(out, b->rc.p, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAgcBatch_ExportState(AspAgcBatch* b, int stream, AspAgcState* out) {
  if (check_stream(b, stream) || !out) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  AGC_TRY(hipMemcpyAsync(out, &b->state[stream], sizeof(AspAgcState), hipMemcpyDeviceToHost, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspAgcBatch_ImportState(AspAgcBatch* b, int stream, const AspAgcState* in) {
  if (check_stream(b, stream) || !in) return ASP_ERR_PARAM;
  // what the kernel indexes with must be in range
  if (!valid_fs(in->fs) || in->initFlag != 42 || in->agcMode < 0 || in->agcMode > 3 || in->Rxx16pos < 0 ||
      in->Rxx16pos > 9 || in->gainTableIdx > 31 || in->targetIdx != 20 || in->inQueue < 0 || in->inQueue > 2 ||
      in->scale != 0 || in->digitalAgc_capacitorFast < 0 || in->digitalAgc_capacitorSlow < 0)
    return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  AGC_TRY(hipMemcpyAsync(&b->state[stream], in, sizeof(AspAgcState), hipMemcpyHostToDevice, b->stream));
  AGC_TRY(hipStreamSynchronize(b->stream));
  b->fs[stream] = in->fs;
  return ASP_OK;
}

int AspAgcBatch_SetStream(AspAgcBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspAgcBatch_Synchronize(AspAgcBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  AGC_TRY(dev_scope_.select(b->device));
  AGC_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

// ---------------------------------------------------------------- layer 1: a batch of one stream
int WebRtcAgc_Create(void** inst) {
  if (!inst) return -1;
  AspAgcBatch* b = nullptr;
  if (AspAgcBatch_Create(&b, 1, 0) != ASP_OK) {
    *inst = nullptr;
    return -1;
  }
  *inst = b;
  return 0;
}
int WebRtcAgc_Free(void* inst) {
  if (!inst) return -1;
  AspAgcBatch_Free((AspAgcBatch*)inst);
  return 0;
}
int WebRtcAgc_Init(void* inst, int32_t lo, int32_t hi, int16_t mode, uint32_t fs) {
  if (!inst) return -1;
  return AspAgcBatch_InitStream((AspAgcBatch*)inst, 0, lo, hi, mode, fs) == 0 ? 0 : -1;
}
int WebRtcAgc_set_config(void* inst, WebRtcAgcConfig c) {
  if (!inst) return -1;
  return AspAgcBatch_set_config_stream((AspAgcBatch*)inst, 0, c) == 0 ? 0 : -1;
}
int WebRtcAgc_get_config(void* inst, WebRtcAgcConfig* c) {
  if (!inst) return -1;
  return AspAgcBatch_get_config_stream((AspAgcBatch*)inst, 0, c) == 0 ? 0 : -1;
}
int WebRtcAgc_AddFarend(void* inst, const int16_t* far, int16_t samples) {
  AspAgcBatch* b = (AspAgcBatch*)inst;
  if (!good_frame(b, 1, samples) || !far) return -1;
  if (AspAgcBatch_AddFarend(b, far, samples, ASP_MEM_HOST) != ASP_OK) return -1;
  return first_return(b);
}
int WebRtcAgc_AddMic(void* inst, int16_t* const* mic, int16_t nb, int16_t n) {
  AspAgcBatch* b = (AspAgcBatch*)inst;
  Planes p;
  if (!good_frame(b, nb, n) || !p.gather(mic, nb, n)) return -1;
  if (AspAgcBatch_AddMic(b, mic[0], p.hi, nb, n, ASP_MEM_HOST) != ASP_OK) return -1;
  p.scatter(mic, nb, n);
  return first_return(b);
}
int WebRtcAgc_VirtualMic(void* inst, int16_t* const* mic, int16_t nb, int16_t n, int32_t level_in, int32_t* level_out) {
  AspAgcBatch* b = (AspAgcBatch*)inst;
  Planes p;
  if (!good_frame(b, nb, n) || !level_out || !p.gather(mic, nb, n)) return -1;
  if (AspAgcBatch_VirtualMic(b, mic[0], p.hi, nb, n, &level_in, level_out, ASP_MEM_HOST) != ASP_OK) return -1;
  p.scatter(mic, nb, n);
  return first_return(b);
}
int WebRtcAgc_Process(void* inst, const int16_t* const* in, int16_t nb, int16_t n, int16_t* const* out, int32_t level_in,
                      int32_t* level_out, int16_t echo, uint8_t* saturation) {
  AspAgcBatch* b = (AspAgcBatch*)inst;
  Planes p, q;
  if (!good_frame(b, nb, n) || !level_out || !saturation || !p.gather(in, nb, n) || !out) return -1;
  for (int k = 0; k < nb; ++k)
    if (!out[k]) return -1;
  if (AspAgcBatch_Process(b, in[0], p.hi, out[0], q.hi, nb, n, &level_in, &echo, level_out, saturation, ASP_MEM_HOST) != ASP_OK)
    return -1;
  q.scatter(out, nb, n);
  return first_return(b);
}

}  // extern "C"
