// The scalar step of AMG-preconditioned conjugate gradients (PCG.m:70-88 with the flexible beta), written once:
// k_kry_dir_spmv / k_kry_dots (ipd_krylov.hip), k_bkry_dir_spmv / k_bkry_dots (ipd_block_krylov.hip) and
// k_pcg_small (ipd_small.hip) call these functions and restate none of them.  Host-clean: no HIP types, no getenv
// -- the CPU test of this header (tests/krylov_plan_driver.cpp) runs what the kernels run, against the restatement
// tests/amg_pcg_ref.py.  Division, square root and comparison only, in the order of PCG.m.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define PCG_HD_INLINE __host__ __device__ __forceinline__
#else
#define PCG_HD_INLINE inline
#endif

// scalar record of one right-hand side (doubles)
enum { SC_DNEW, SC_DOLD, SC_ALPHA, SC_BETA, SC_D0, SC_IT, SC_RES, SC_STOP, SC_N };

// ---- the rules over values (k_pcg_small keeps its scalars in registers) ----
// flexible (Polak-Ribiere) beta = (r'w - r'w_old) / delta_old                                     PCG.m:82
PCG_HD_INLINE double pcg_beta(double dn, double s_wo, double delta_old) { return (dn - s_wo) / delta_old; }
// sqrt|delta_new / delta_0|: NaN for delta_0 = 0 (a padding column), |.| for a negative delta_new    :85 / :88
PCG_HD_INLINE double pcg_res(double dn, double d0) { return sqrt(fabs(dn / d0)); }

// ---- the same rules over a record S[SC_N] ----
// before the update: delta_old = delta_new, alpha = delta_old / p'q                                  :77-78
PCG_HD_INLINE void pcg_step_alpha(double* S, double pq) {
    const double dn = S[SC_DNEW];
    S[SC_DOLD] = dn;
    S[SC_ALPHA] = dn / pq;
}

// after a preconditioner application, dn = r'w: the first form (FIRST, :70-72: delta_0 = dn, it = 0, beta = 0) and
// the later one (s_wo = r'w_old; beta, it + 1).  Both leave delta_new, it, res and the stop flag; true: go on.
template <bool FIRST>
PCG_HD_INLINE bool pcg_step(double* S, double dn, double s_wo, double maxit, double tol2) {
    double d0, itv;
    if (FIRST) {
        d0 = dn;
        itv = 0.0;
        S[SC_D0] = d0;
        S[SC_BETA] = 0.0;
    } else {
        d0 = S[SC_D0];
        S[SC_BETA] = pcg_beta(dn, s_wo, S[SC_DOLD]);
        itv = S[SC_IT] + 1.0;                                                                       // :84
    }
    S[SC_DNEW] = dn;                                                                                // :81
    S[SC_IT] = itv;
    S[SC_RES] = pcg_res(dn, d0);
    // the loop test: false at once for maxit = 0 and for delta_0 = 0; tol2 = 0 runs to maxit         :76
    // (written here and not as a function over values: called through one, the compiler orders the two
    // comparisons' operands differently in k_kry_dots and k_bkry_dots; k_pcg_small, whose count is an int,
    // restates this one line)
    const bool go = itv < maxit && dn > tol2 * d0;
    S[SC_STOP] = go ? 0.0 : 1.0;
    return go;
}
