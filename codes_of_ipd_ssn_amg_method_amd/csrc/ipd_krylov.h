// What the kernels of the single-vector AMG-PCG (ipd_krylov.hip) and of its block form (ipd_block_krylov.hip)
// share: the fixed-order last-arriver reduction, and the scalar step (ipd_pcg_step.h) and host rules
// (ipd_krylov_plan.h) that come with it.
#pragma once

#include "ipd_amg_internal.h"

#include "ipd_cycle_dev.h"
#include "ipd_krylov_plan.h"
#include "ipd_pcg_step.h"

// Wave 0 of every workgroup calls this after thread 0 stored the workgroup's partials; true (in wave
// 0 only) in the workgroup that arrives last, which then sees every partial and has reset the ticket.
__device__ __forceinline__ bool kry_last_arrival(unsigned* cnt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // keep: the fence's own wait can be dropped
    unsigned t = 0;
    if (threadIdx.x == 0) t = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t != gridDim.x - 1) return false;
    if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

// sum of part[0], part[stride], ... (n terms) in a fixed order, result in every lane of wave 0
__device__ __forceinline__ double kry_sum_parts(const double* part, int n, int stride) {
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += 64) s += part[(size_t)i * stride];
    return wave_sum(s);
}

static inline void pcg_opts_of(const ipd_pcg_opts* o, double* tol, long long* maxit) {
    IPD_REQUIRE(pcg_opts_rule(o, tol, maxit), IPD_E_ARG,
                "AMG-PCG: pcg_options.precd must be unset (the hierarchy preconditions)");
}
