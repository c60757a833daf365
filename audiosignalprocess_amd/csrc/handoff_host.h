// handoff_host.h -- the host side of the hand-off build (the protocol: handoff.h), shared by ns_api.hip,
// aec_api.hip and bt_api.hip: the per-stream step counters and the abort word of one batch, the count of steps
// enqueued, and the check after a synchronisation.  Each API reports a timeout with its own code and message.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

// steps per launch of the hand-off build (grid y)
constexpr int kHandoffMaxSteps = 64;

// The hand-off build's default: on unless the environment variable `var` is set and starts with '0'.
inline bool handoff_env_default(const char* var) {
  const char* e = getenv(var);
  return !(e && e[0] == '0');
}

struct HandoffSync {
  unsigned* seq = nullptr;    // [S] completed hand-off steps per stream (== count between calls; inside a launch a
                              // kernel may advance it by several steps at once: only the value after a launch counts)
  unsigned* abort = nullptr;  // 16 B: word 0 != 0 after a wait timed out
  unsigned count = 0;         // hand-off steps enqueued so far
  bool unchecked = false;     // hand-off launches enqueued since the abort word was last read

  // First use: allocate and clear the counters on the batch's stream.
  hipError_t ensure(int S, hipStream_t stream) {
    if (seq) return hipSuccess;
    hipError_t e;
    if ((e = hipMalloc((void**)&seq, (size_t)S * sizeof(unsigned))) != hipSuccess) return e;
    if ((e = hipMalloc((void**)&abort, 16)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(seq, 0, (size_t)S * sizeof(unsigned), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(abort, 0, 16, stream)) != hipSuccess) return e;
    count = 0;
    return hipSuccess;
  }
  // m more steps of every stream have been enqueued.
  void enqueued(int m) {
    count += (unsigned)m;
    unchecked = true;
  }
  // After the batch's stream has been synchronised: did a hand-off wait time out?  (It cannot while the launches
  // of one batch run as enqueued; a timeout means steps were skipped.)  If so, the counters are put back in step
  // and *timed_out is set; the caller fails loudly.
  hipError_t check(int S, bool* timed_out) {
    *timed_out = false;
    if (!unchecked) return hipSuccess;
    unchecked = false;
    unsigned a = 0;
    hipError_t e;
    if ((e = hipMemcpy(&a, abort, sizeof a, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if (a == 0) return hipSuccess;
    std::vector<unsigned> s((size_t)S, count);
    if ((e = hipMemcpy(seq, s.data(), s.size() * sizeof(unsigned), hipMemcpyHostToDevice)) != hipSuccess) return e;
    if ((e = hipMemset(abort, 0, 16)) != hipSuccess) return e;
    *timed_out = true;
    return hipSuccess;
  }
  void release() {
    if (seq) (void)hipFree(seq);
    if (abort) (void)hipFree(abort);
    seq = abort = nullptr;
  }
};
