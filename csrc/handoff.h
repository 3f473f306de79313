// The fence-free last-arriver hand-off of the BatchNorm statistics launch (csrc/bn.hip).
//
// Hand-off (cdna_hip_programming.md Guideline 16, sc1 form): every slab word is stored write-through
// (relaxed agent-scope atomic store = sc1) and drained by every storing wave before the barrier; lane 0
// then draws a ticket.  The last of `n` arrivers reads the slabs with sc1 loads, so neither side pays an
// agent-scope release (L2 write-back) or acquire.  The last arriver re-arms the counter for the next
// launch.  Every sum runs in a fixed order (tile order, then group order): deterministic.
// Memory-model note: the ordering this relies on -- write-through (sc1) stores drained by
// s_waitcnt vmcnt(0) in every storing wave before a relaxed agent-scope ticket RMW, then sc1 loads in
// the last arriver -- is the gfx950 hand-off form of cdna_hip_programming.md Guideline 16 (R1, counter
// variant) and MI355X_MICROARCH.md's visibility rules, not a C++-memory-model happens-before: the
// vmcnt drain is what makes the stores globally performed before the ticket.  This header is gfx950
// only (the build targets nothing else); a port would put release / acquire on the ticket instead.
#pragma once
#include "common.h"

namespace dfa {

__device__ __forceinline__ void st_sc1(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_sc1(const float* p) {
  return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ bool last_arriver(unsigned* counter, unsigned n, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its sc1 stores
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned tk = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = (tk == n - 1) ? 1 : 0;
    if (*flag) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the loads below the ticket
  return *flag != 0;
}

}  // namespace dfa
