// api_common.h -- the host-side plumbing that every *_api.hip shares, and nothing else: the error record,
// the device scope, and the growable device staging buffer.  Host-only, header-only.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdio.h>

#include "asp_ns.h"  // ASP_OK / ASP_ERR_*

// one copy per library, none of it exported: the library's dynamic symbols are its C-ABI only
#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------ error record
// The calling thread's last failure text, one for the whole library (AspNs_last_error returns it).
inline thread_local char g_asp_err[512] = "";
inline const char* asp_last_error() { return g_asp_err; }

// Records "<what>[: <HIP error string>]" and returns `code`; with a tag, also prints "<tag>: <text>" on stderr.
inline int asp_fail(const char* tag, int code, const char* what, hipError_t e = hipSuccess) {
  if (e != hipSuccess)
    snprintf(g_asp_err, sizeof g_asp_err, "%s: %s", what, hipGetErrorString(e));
  else
    snprintf(g_asp_err, sizeof g_asp_err, "%s", what);
  if (tag) fprintf(stderr, "%s: %s\n", tag, g_asp_err);
  return code;
}

#define ASP_TRY(tag, expr)                                              \
  do {                                                                  \
    hipError_t e_ = (expr);                                             \
    if (e_ != hipSuccess) return asp_fail(tag, ASP_ERR_HIP, #expr, e_); \
  } while (0)

// ------------------------------------------------------------------ device scope
// Every entry point of the C-ABI selects its batch's device for its HIP calls through this object, and only
// through it; the caller's current device is put back when the entry point returns, so that a host thread
// that drives batches on several GPUs (or mixes this library with its own HIP code) never finds its device
// changed.
struct AspDeviceScope {
  int prev = -1;
  AspDeviceScope() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~AspDeviceScope() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
  AspDeviceScope(const AspDeviceScope&) = delete;
  AspDeviceScope& operator=(const AspDeviceScope&) = delete;

  // the device of an existing handle
  hipError_t select(int device) { return hipSetDevice(device); }

  // Create and the handle-less entry points: is there a HIP device, is the ordinal in range, select it.
  // An ordinal out of range returns `bad_ordinal`: ASP_ERR_PARAM or ASP_ERR_NO_DEVICE, as the module's ABI
  // has it (with ASP_ERR_NO_DEVICE the text is `no_device` as well).
  int select(const char* tag, int device, int bad_ordinal, const char* no_device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return asp_fail(tag, ASP_ERR_NO_DEVICE, no_device);
    if (device < 0 || device >= n)
      return asp_fail(tag, bad_ordinal, bad_ordinal == ASP_ERR_NO_DEVICE ? no_device : "device ordinal out of range");
    ASP_TRY(tag, hipSetDevice(device));
    return ASP_OK;
  }
};

// ------------------------------------------------------------------ staging
// A device buffer that grows to the largest size asked for (staging for host-memory callers).
struct AspStage {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (cap >= bytes) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

#pragma GCC visibility pop
