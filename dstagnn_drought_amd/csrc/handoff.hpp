// handoff.hpp — the in-kernel fold's ticket hand-off: the ONLY place the protocol is written.
//
// Workgroups of one launch hand partial sums to whichever of them arrives last (MI355X_MICROARCH.md,
// inter-workgroup visibility, "Valid forms"; cdna_hip_programming.md, Guideline 16).  The order of
// the steps IS the correctness argument; none may be left out or moved:
//   1. producers store their partials sc1 (st_agent: agent-scope relaxed atomics)
//   2. every storing wave drains them (s_waitcnt vmcnt(0))
//   3. a workgroup barrier
//   4. ONE lane's agent-scope ticket add on a zero-armed counter
//   5. the workgroup whose add came last takes an agent-scope ACQUIRE, waits for its invalidate
//      (s_waitcnt vmcnt(0)), and a barrier holds its other waves behind that
//   6. it sums the partials in a fixed order (deterministic) and re-arms the counter to 0
// No release fence on the producers: it would write back the XCD's whole L2, and sc1 stores already
// bypass that L2 (written through, the line dropped), so after the drain they are where any other
// XCD's sc1 or post-acquire load finds them.  The acquire stays: it invalidates the last arrival's
// L1 (only the winners pay it), so the reads do not rest on the measured sc1-load table, whose row
// assumes one workgroup per CU.
// The re-arm comes right after the acquire: all n adds have happened by then.  Every user draws from
// one per-stream pool (stream_counters), so each must leave its tickets at zero for the next.
#pragma once
#include <hip/hip_runtime.h>

// sc1 (agent-scope relaxed) load / store of a partial
__device__ __forceinline__ float ld_agent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... of an fp64 partial: one aligned 8-byte access, never two halves
__device__ __forceinline__ double ld_agent(const double* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(double* p, double v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ... of an int64 partial (an exact count)
__device__ __forceinline__ long long ld_agent(const long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(long long* p, long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one lane: draw a ticket among n arrivals (step 4, no fence); true for the last arrival
__device__ __forceinline__ bool ticket_draw(int* cnt, int n) { return atomicAdd(cnt, 1) == n - 1; }
// one lane of the last arrival: agent acquire, then wait for the invalidate to complete (step 5;
// the caller's barrier holds the other waves behind it)
__device__ __forceinline__ void ticket_acquire() {
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// one lane of the last arrival, after its acquire: the counter back to 0 for the stream's next user
__device__ __forceinline__ void ticket_rearm(int* cnt) {
  __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Steps 2-5 and the re-arm for a whole (1-D) workgroup, called by all its threads after their
// st_agent stores: true, uniformly, in the last of the n arrivals on *cnt.  flag: a word in LDS.
__device__ __forceinline__ bool last_arrival(int* cnt, int n, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool last = ticket_draw(cnt, n);
    if (last) {
      ticket_acquire();
      ticket_rearm(cnt);
    }
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

// sum of the n partials src[k * row_stride] in index order (step 6): chunks of G sc1 loads issued
// before the chunk's first add (one memory round trip per chunk: sc1 loads are served beyond the
// XCD's L2), chunk after chunk into one accumulator
template <int G, typename T>
__device__ __forceinline__ T sum_rows_agent(const T* src, int64_t row_stride, int n) {
  T v = T(0);
  for (int k0 = 0; k0 < n; k0 += G) {
    T u[G];
#pragma unroll
    for (int k = 0; k < G; ++k) u[k] = k0 + k < n ? ld_agent(src + (k0 + k) * row_stride) : T(0);
#pragma unroll
    for (int k = 0; k < G; ++k) v += u[k];
  }
  return v;
}
