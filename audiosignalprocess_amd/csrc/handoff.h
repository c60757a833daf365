// handoff.h -- the device side of the hand-off build, shared by ns_kernels1.hip, ns_kernels2.hip,
// aec_kernels.hip and bt_kernels8.hip (the host side: handoff_host.h).
//
// One launch carries up to kHandoffMaxSteps consecutive steps of a whole batch: blockIdx.y is the step,
// blockIdx.x the group of streams.  Workgroups are dispatched in linear grid order (x fastest), so every
// workgroup of step j has been dispatched before the first one of step j + 1: the wave that takes stream s
// in step j + 1 may WAIT for the wave that has stream s in step j -- that wave is resident or done, whatever
// else runs on the chip (the forward-progress argument of a decoupled look-back scan).  The grid's x extent is
// a multiple of 8, so that (with workgroups dealt round-robin to the 8 XCDs) both come from the same XCD's
// in-order share of the grid.
//
// The chunked form (ns_kernels1.hip, NsFlowArgs::walk): blockIdx.y is a CHUNK of C consecutive steps, and workgroup
// (x, c) walks steps c C .. min(steps, (c + 1) C) - 1 of its streams in a loop.  Only the chunk's first step waits
// (for the wave of chunk c - 1, dispatched earlier: the same argument as above).  Nobody else may touch the stream's
// state before the walk ends, so between two steps of its own the wave neither drains nor publishes: it keeps the
// hot part of the state on the chip (an LDS image, copied in behind the wait), and after the walk's last step writes
// it back, drains, and publishes seq[s] ONCE, as the step count at the walk's end.  seq[s] counts the steps stream s
// has completed AND handed back to memory: it advances once per walk (by C, or by what is left of the launch), state
// in memory is consistent at every value seq[s] takes, and the only value the host may rely on is the one after a
// launch (handoff_host.h).  What stays in memory inside a walk and is read back there (rare paths) waits for the
// wave's own outstanding stores first.  With C = steps no workgroup waits for another one of the launch (only for the
// previous launch, which stream order has finished): nothing then rests on dispatch order.  C = 1 is the form above
// with a copy in and a copy out around every step.  The host picks C (ns_api.hip, flow_walk).
//
// What orders the two is a per-stream step counter in memory, seq[s]:
//   * the wave that has finished step k of stream s (chunked form: the last step k of its walk) drains every store it
//     issued (handoff_drain: s_waitcnt vmcnt(0)), then one lane stores seq[s] = k + 1 (handoff_publish);
//   * the wave of step k + 1 polls seq[s] (handoff_wait) before its first access to what is handed off.
// Every access to what a stream's steps hand each other is an sc1 access: write-through stores, loads that
// bypass the CU's L1 (the buffer intrinsics with kSc1, or agent-scope relaxed atomics).  This is the form
// MI355X_MICROARCH.md ("Workgroup dispatch, XCD placement & inter-workgroup visibility") lists for hand-offs
// without an agent-scope fence per wave.  What is not handed off (frames in / out, constant tables) stays plain.
//
// The wait is bounded: a wave that has polled kHandoffSpinLimit times without a match stores 1 + id into the
// abort word (id names the stream or workgroup that waited) and gives up; every later wait checks the abort
// word once per kHandoffAbortPoll polls and gives up as well.  The grid then drains, and the host reports the
// failure after its next synchronisation (handoff_host.h, HandoffSync::check).
#pragma once
#include <hip/hip_runtime.h>

namespace asphandoff {

typedef __attribute__((address_space(1))) unsigned gu32;
constexpr int kSc1 = 16;                      // cache-policy operand of the buffer intrinsics: sc1
constexpr unsigned kHandoffAbortPoll = 64;    // polls between two reads of the abort word (a power of two)
constexpr unsigned kHandoffSpinLimit = 1u << 17;  // polls before a wait gives up (~0.1 s)
constexpr int kHandoffSleep = 2;              // s_sleep operand between two polls

// The kernel arguments every hand-off build carries; each kernel's own struct embeds them.  (The step number
// `want` stays in the kernel's struct, next to these: a 24-byte base would move the fields behind it.)
struct HandoffArgs {
  unsigned* seq;      // [num_streams]: hand-off steps stream s has completed
  unsigned* abort_w;  // != 0: a wait timed out (1 + id)
};

// One poll that did not match: false when the wait is given up (abort word set by another wave, or by this one
// after kHandoffSpinLimit polls); otherwise sleeps before the next poll.
__device__ __forceinline__ bool handoff_spin(const HandoffArgs& h, unsigned& spins, unsigned id, int lane) {
  ++spins;
  if ((spins & (kHandoffAbortPoll - 1u)) == 0u) {
    const unsigned a = __hip_atomic_load((const gu32*)h.abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__builtin_amdgcn_readfirstlane((int)a) != 0) return false;
  }
  if (spins > kHandoffSpinLimit) {
    if (lane == 0) __hip_atomic_store((gu32*)h.abort_w, 1u + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
  }
  __builtin_amdgcn_s_sleep(kHandoffSleep);
  return true;
}

// Uniform form (one stream per wave): wait until seq[stream] == want.  False: given up.
__device__ __forceinline__ bool handoff_wait(const HandoffArgs& h, unsigned want, int stream, int lane) {
  const gu32* f = (const gu32*)(h.seq + stream);
  unsigned spins = 0;
  for (;;) {
    const unsigned v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((unsigned)__builtin_amdgcn_readfirstlane((int)v) == want) break;
    if (!handoff_spin(h, spins, (unsigned)stream, lane)) return false;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the poll
  return true;
}

// Per-lane form: each lane polls its own word seq[word]; lanes with `live` false have nothing to wait for.  The
// wait ends when every lane's word has reached `want`.  The abort word gets 1 + id.  False: given up.
__device__ __forceinline__ bool handoff_wait_lanes(const HandoffArgs& h, unsigned want, size_t word, bool live,
                                                   unsigned id, int lane) {
  const gu32* f = (const gu32*)(h.seq + word);
  unsigned spins = 0;
  for (;;) {
    const unsigned v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__all(v == want || !live)) break;
    if (!handoff_spin(h, spins, id, lane)) return false;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the poll
  return true;
}

// Every store this wave has issued is complete: what it hands off is visible before the counter moves.
__device__ __forceinline__ void handoff_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Step `want` is done: *word (a stream's seq entry) = want + 1.  After handoff_drain; the caller picks the lanes.
__device__ __forceinline__ void handoff_publish(unsigned* word, unsigned want) {
  __hip_atomic_store((gu32*)word, want + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sc1 accesses through a buffer resource: `voff` the lane's byte offset, `soff` a wave-uniform byte offset.
typedef float f32x2v __attribute__((ext_vector_type(2)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float sc1_load1(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, soff, kSc1));
}
__device__ __forceinline__ float2 sc1_load2(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  const f32x2v v = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rs, voff, soff, kSc1));
  return make_float2(v.x, v.y);
}
__device__ __forceinline__ float4 sc1_load4(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  const f32x4v v = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, kSc1));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void sc1_store1(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float x) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), rs, voff, soff, kSc1);
}
__device__ __forceinline__ void sc1_store2(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float a, float b) {
  const f32x2v v = {a, b};
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, v), rs, voff, soff, kSc1);
}
__device__ __forceinline__ void sc1_store4(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float4 x) {
  const f32x4v v = {x.x, x.y, x.z, x.w};
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), rs, voff, soff, kSc1);
}

}  // namespace asphandoff
