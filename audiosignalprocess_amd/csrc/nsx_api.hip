// nsx_api.hip -- host side of include/asp_nsx.h: the batch handle (every stream's AspNsxState in HBM), the
// per-call validation, the constant tables, and the reference's WebRtcNsx_* as a batch of one stream.
// No CPU fallback.
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "api_common.h"
#include "nsx_layout.h"

namespace aspnsx {
hipError_t launch_frames(AspNsxState* st, const NsxTables* T, int S, int F, int n, int nb, const int16_t* low_in,
                         const int16_t* high_in, int16_t* low_out, int16_t* high_out, hipStream_t stream);
hipError_t launch_control(AspNsxState* st, int first, int count, int op, int arg, hipStream_t stream);
}  // namespace aspnsx

using namespace aspnsx;

#define nsx_fail(...) asp_fail("asp_nsx", __VA_ARGS__)
#define NSX_TRY(x) ASP_TRY("asp_nsx", x)

namespace {
thread_local int g_nsx_refused = 0;
bool valid_fs(uint32_t fs) { return fs == 8000 || fs == 16000 || fs == 32000 || fs == 48000; }
}  // namespace

struct AspNsxBatch {
  int S = 0, device = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  AspNsxState* state = nullptr;  // [S]
  NsxTables* tables = nullptr;
  std::vector<uint32_t> fs;  // per stream; 0: not initialised
  AspStage s_li, s_hi, s_lo, s_ho;  // staging for host-memory callers
};

namespace {
int check_stream(AspNsxBatch* b, int s) { return (b && s >= 0 && s < b->S) ? ASP_OK : ASP_ERR_PARAM; }

int control(AspNsxBatch* b, int first, int count, int op, int arg) {
  AspDeviceScope dev_scope_;
  NSX_TRY(dev_scope_.select(b->device));
  NSX_TRY(launch_control(b->state, first, count, op, arg, b->stream));
  return ASP_OK;
}

int run_frames(AspNsxBatch* b, int F, const int16_t* li, const int16_t* hi, int16_t* lo, int16_t* ho, int nb, int n,
               int mem) {
  if (!b || F < 0 || (mem != ASP_MEM_HOST && mem != ASP_MEM_DEVICE)) return ASP_ERR_PARAM;
  if ((n != 80 && n != 160) || nb < 1 || nb > 3 || !li || !lo) return ASP_ERR_PARAM;
  if (nb > 1 && (!hi || !ho)) return ASP_ERR_PARAM;
  for (int s = 0; s < b->S; ++s) {
    if (!b->fs[s]) return nsx_fail(ASP_ERR_STATE, "AspNsxBatch: stream not initialised");
    if ((b->fs[s] == 8000 ? 80 : 160) != n)
      return nsx_fail(ASP_ERR_STATE, "AspNsxBatch: a stream was initialised for the other frame length");
  }
  if (F == 0) return ASP_OK;
  const int S = b->S;
  const size_t lb = (size_t)F * S * n * sizeof(int16_t), hb = lb * (nb - 1);
  AspDeviceScope dev_scope_;
  NSX_TRY(dev_scope_.select(b->device));
  const int16_t *d_li = li, *d_hi = hi;
  int16_t *d_lo = lo, *d_ho = ho;
  if (mem == ASP_MEM_HOST) {
    NSX_TRY(b->s_li.reserve(lb));
    NSX_TRY(b->s_lo.reserve(lb));
    NSX_TRY(hipMemcpyAsync(b->s_li.p, li, lb, hipMemcpyHostToDevice, b->stream));
    d_li = (const int16_t*)b->s_li.p;
    d_lo = (int16_t*)b->s_lo.p;
    if (nb > 1) {
      NSX_TRY(b->s_hi.reserve(hb));
      NSX_TRY(b->s_ho.reserve(hb));
      NSX_TRY(hipMemcpyAsync(b->s_hi.p, hi, hb, hipMemcpyHostToDevice, b->stream));
      d_hi = (const int16_t*)b->s_hi.p;
      d_ho = (int16_t*)b->s_ho.p;
    }
  }
  NSX_TRY(launch_frames(b->state, b->tables, S, F, n, nb, d_li, d_hi, d_lo, d_ho, b->stream));
  if (mem == ASP_MEM_HOST) {
    NSX_TRY(hipMemcpyAsync(lo, d_lo, lb, hipMemcpyDeviceToHost, b->stream));
    if (nb > 1) NSX_TRY(hipMemcpyAsync(ho, d_ho, hb, hipMemcpyDeviceToHost, b->stream));
  }
  NSX_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}
}  // namespace

extern "C" {

size_t AspNsx_state_size(void) { return sizeof(AspNsxState); }
int AspNsx_last_refused(void) { return g_nsx_refused; }

int AspNsxBatch_Free(AspNsxBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  (void)dev_scope_.select(b->device);
  if (b->own_stream) (void)hipStreamSynchronize(b->own_stream);
  void* bufs[] = {b->state, b->tables, b->s_li.p, b->s_hi.p, b->s_lo.p, b->s_ho.p};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  if (b->own_stream) (void)hipStreamDestroy(b->own_stream);
  delete b;
  return ASP_OK;
}

int AspNsxBatch_Create(AspNsxBatch** out, int num_streams, int device) {
  if (!out || num_streams < 1) return ASP_ERR_PARAM;
  *out = nullptr;
  AspDeviceScope dev_scope_;
  if (int rc = dev_scope_.select("asp_nsx", device, ASP_ERR_NO_DEVICE, "AspNsxBatch_Create: no HIP device")) return rc;
  AspNsxBatch* b = new AspNsxBatch;
  b->S = num_streams;
  b->device = device;
  b->fs.assign(num_streams, 0);
  static NsxTables T;
  build_tables(&T);
  hipError_t e = hipStreamCreateWithFlags(&b->own_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc((void**)&b->state, sizeof(AspNsxState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMalloc((void**)&b->tables, sizeof(NsxTables));
  if (e == hipSuccess) e = hipMemset(b->state, 0, sizeof(AspNsxState) * (size_t)num_streams);
  if (e == hipSuccess) e = hipMemcpy(b->tables, &T, sizeof T, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    AspNsxBatch_Free(b);
    return nsx_fail(ASP_ERR_HIP, "AspNsxBatch_Create", e);
  }
  b->stream = b->own_stream;
  *out = b;
  return ASP_OK;
}

int AspNsxBatch_num_streams(const AspNsxBatch* b) { return b ? b->S : ASP_ERR_PARAM; }

int AspNsxBatch_Init(AspNsxBatch* b, uint32_t fs) {
  if (!b || !valid_fs(fs)) return ASP_ERR_PARAM;
  int rc = control(b, 0, b->S, 0, (int)fs);
  if (rc == ASP_OK) b->fs.assign(b->S, fs);
  return rc;
}
int AspNsxBatch_InitStream(AspNsxBatch* b, int stream, uint32_t fs) {
  if (check_stream(b, stream) || !valid_fs(fs)) return ASP_ERR_PARAM;
  int rc = control(b, stream, 1, 0, (int)fs);
  if (rc == ASP_OK) b->fs[stream] = fs;
  return rc;
}
int AspNsxBatch_set_policy(AspNsxBatch* b, int mode) {
  if (!b || mode < 0 || mode > 3) return ASP_ERR_PARAM;
  return control(b, 0, b->S, 1, mode);
}
int AspNsxBatch_set_policy_stream(AspNsxBatch* b, int stream, int mode) {
  if (check_stream(b, stream) || mode < 0 || mode > 3) return ASP_ERR_PARAM;
  return control(b, stream, 1, 1, mode);
}

int AspNsxBatch_Process(AspNsxBatch* b, const int16_t* li, const int16_t* hi, int16_t* lo, int16_t* ho, int nb, int n,
                        int mem) {
  return run_frames(b, 1, li, hi, lo, ho, nb, n, mem);
}
int AspNsxBatch_ProcessFrames(AspNsxBatch* b, int F, const int16_t* li, const int16_t* hi, int16_t* lo, int16_t* ho,
                              int nb, int n, int mem) {
  return run_frames(b, F, li, hi, lo, ho, nb, n, mem);
}

int AspNsxBatch_ExportState(AspNsxBatch* b, int stream, AspNsxState* out) {
  if (check_stream(b, stream) || !out) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  NSX_TRY(dev_scope_.select(b->device));
  NSX_TRY(hipMemcpyAsync(out, &b->state[stream], sizeof(AspNsxState), hipMemcpyDeviceToHost, b->stream));
  NSX_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

int AspNsxBatch_ImportState(AspNsxBatch* b, int stream, const AspNsxState* in) {
  if (check_stream(b, stream) || !in) return ASP_ERR_PARAM;
  if (!valid_fs(in->fs) || in->initFlag != 1 || in->aggrMode < 0 || in->aggrMode > 3 ||
      in->anaLen != (in->fs == 8000 ? 128 : 256) || in->stages != (in->fs == 8000 ? 7 : 8) ||
      in->anaLen2 != in->anaLen / 2 || in->magnLen != in->anaLen2 + 1 ||
      in->blockLen10ms != (in->fs == 8000 ? 80 : 160) || in->noiseEstCounter[0] < 0 || in->noiseEstCounter[0] > 200 ||
      in->noiseEstCounter[1] < 0 || in->noiseEstCounter[1] > 200 || in->noiseEstCounter[2] < 0 ||
      in->noiseEstCounter[2] > 200 || in->normData < 0 || in->normData > 15)
    return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  NSX_TRY(dev_scope_.select(b->device));
  NSX_TRY(hipMemcpyAsync(&b->state[stream], in, sizeof(AspNsxState), hipMemcpyHostToDevice, b->stream));
  NSX_TRY(hipStreamSynchronize(b->stream));
  b->fs[stream] = in->fs;
  return ASP_OK;
}

int AspNsxBatch_SetStream(AspNsxBatch* b, void* hip_stream) {
  if (!b) return ASP_ERR_PARAM;
  b->stream = hip_stream ? (hipStream_t)hip_stream : b->own_stream;
  return ASP_OK;
}

int AspNsxBatch_Synchronize(AspNsxBatch* b) {
  if (!b) return ASP_ERR_PARAM;
  AspDeviceScope dev_scope_;
  NSX_TRY(dev_scope_.select(b->device));
  NSX_TRY(hipStreamSynchronize(b->stream));
  return ASP_OK;
}

// ---------------------------------------------------------------- layer 1: a batch of one stream
int WebRtcNsx_Create(NsxHandle** inst) {
  if (!inst) return -1;
  AspNsxBatch* b = nullptr;
  if (AspNsxBatch_Create(&b, 1, 0) != ASP_OK) {
    *inst = nullptr;
    return -1;
  }
  *inst = (NsxHandle*)b;
  return 0;
}
int WebRtcNsx_Free(NsxHandle* inst) {
  if (!inst) return -1;
  AspNsxBatch_Free((AspNsxBatch*)inst);
  return 0;
}
int WebRtcNsx_Init(NsxHandle* inst, uint32_t fs) {
  if (!inst) return -1;
  return AspNsxBatch_InitStream((AspNsxBatch*)inst, 0, fs) == ASP_OK ? 0 : -1;
}
int WebRtcNsx_set_policy(NsxHandle* inst, int mode) {
  if (!inst) return -1;
  return AspNsxBatch_set_policy_stream((AspNsxBatch*)inst, 0, mode) == ASP_OK ? 0 : -1;
}
void WebRtcNsx_Process(NsxHandle* inst, const short* const* in, int nb, short* const* out) {
  AspNsxBatch* b = (AspNsxBatch*)inst;
  g_nsx_refused = 1;
  if (!b || !in || !out || nb < 1 || nb > 3 || !b->fs[0]) {
    nsx_fail(ASP_ERR_STATE, "WebRtcNsx_Process refused: NULL argument, handle not initialised, or num_bands outside 1..3");
    return;
  }
  const int n = b->fs[0] == 8000 ? 80 : 160;
  // the bands as planes [nb - 1][1][n]
  int16_t hi[2 * 160], ho[2 * 160];
  for (int k = 1; k < nb; ++k) {
    if (!in[k] || !out[k]) return;
    memcpy(hi + (k - 1) * n, in[k], n * sizeof(int16_t));
  }
  if (!in[0] || !out[0]) return;
  if (run_frames(b, 1, in[0], nb > 1 ? hi : nullptr, out[0], nb > 1 ? ho : nullptr, nb, n, ASP_MEM_HOST) != ASP_OK) return;
  for (int k = 1; k < nb; ++k) memcpy(out[k], ho + (k - 1) * n, n * sizeof(int16_t));
  g_nsx_refused = 0;
}

}  // extern "C"
