// The scalar script of the drivers: every decision of APD_SsN_Class{1,2}.m and warmup_class{1,2}.m that the host
// takes between two passes, written once.  ipd_driver.hip (apd_iterate, the ABI), ipd_apd_passes.hip and
// ipd_apd_warm.hip call these functions and hold no copy of them.  Host-clean: no HIP types, no getenv -- the CPU
// tests of this header (tests/apd_script_driver.cpp; tests/gap_rule_driver.cpp for the stopping rule on the certified
// gap, which ipd_bracket.hip and ipd_apd_run's probe take from here) run what the library runs.  Every expression keeps
// the order of operations of the scripts (the library is built with -ffp-contract=off, and so are the tests).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "ipd_apd_geo.h"

#if defined(__HIPCC__)
#define APD_HD_INLINE __host__ __device__ __forceinline__
#else
#define APD_HD_INLINE inline
#endif

// ---------------------------------------------------------------------------
// step scalars                                                 Class1 :113-123, Class2 :110-117
// ---------------------------------------------------------------------------
struct ApdStep {
    double ak, bk1, tk;
};

static inline ApdStep apd_step(int k, double bk) {
    const double kk = (double)k;
    ApdStep s;
    s.ak = std::sqrt(kk * kk * bk);
    s.bk1 = bk / (1.0 + s.ak);
    s.tk = bk * (1.0 + s.ak) / (s.ak * s.ak);
    return s;
}

static inline double apd_ssn_tol(int k, double bk1, double tol1) {                // :123
    return std::max(bk1 / ((double)k * (double)k), tol1);
}

// below this change of |Fk| the Newton loop has stalled                          :219 / Class2 :207
static inline double apd_stall_bound(bool cls2, double ssn_tol) { return cls2 ? ssn_tol : ssn_tol / 100.0; }

// ---------------------------------------------------------------------------
// warm start                                      warmup_class1.m:57-77 / warmup_class2.m:57-85
// ---------------------------------------------------------------------------
struct WarmScal {   // what the warm start's kernels take
    double ak, gk, muf, etafk, sgk, ibk, akbk, ak2, tt_etafk /* etafk+tt */, prox_scale /* ak^2/etagk */;
    double gkmu;  // gk + muf*ak
    double iak1;  // 1+ak
};

struct WarmStep {
    WarmScal s;
    double sg;         // shift of invAAt / invHHt
    double gk1, bk1;   // gk, bk of the next iteration
};

static inline WarmStep apd_warm_step(double gk, double bk, double muf) {
    const double ak = bk, bk1 = bk / (1.0 + ak);
    const double gk1 = (gk + muf * ak) / (1.0 + ak);
    const double etafk = (1.0 + ak) * gk + muf * ak;
    const double sgk = 1.0 / bk1, etagk = (1.0 + ak) * bk;
    const double tt = sgk * ak * ak;
    WarmStep w;
    w.sg = 1.0 + etafk / tt;
    w.gk1 = gk1;
    w.bk1 = bk1;
    WarmScal& s = w.s;
    s.ak = ak;
    s.gk = gk;
    s.muf = muf;
    s.etafk = etafk;
    s.sgk = sgk;
    s.ibk = 1.0 / bk;
    s.akbk = ak / bk;
    s.ak2 = ak * ak;
    s.tt_etafk = etafk + tt;
    s.prox_scale = ak * ak / etagk;
    s.gkmu = gk + muf * ak;
    s.iak1 = 1.0 + ak;
    return w;
}

// ---------------------------------------------------------------------------
// merit                                                                          :182-187
// ---------------------------------------------------------------------------
// cFk = bk1/2 |lk|^2 - wlk'lk + tk/2 |prox(zk)|^2, or with prob 3 (class 1) tk/2 (|zk|^2 - |zk - prox(zk)|^2).
// The one statement of it: the host's line search, ipd_apd_eval / ipd_apd_eval_trial and k_merit_fin call it.
APD_HD_INLINE double apd_merit_value(bool merit3, double bk1, double tk, double lam2, double wlk_lam, double prox2,
                                     double z2, double zmp2) {
    const double f0 = bk1 / 2.0 * lam2 - wlk_lam;
    return merit3 ? f0 + 0.5 * tk * (z2 - zmp2) : f0 + 0.5 * tk * prox2;
}

// ---------------------------------------------------------------------------
// line search                                                                    :189-211
// ---------------------------------------------------------------------------
constexpr int MK = 8;   // trial steps whose merits one pass over wk evaluates (apd_merit)

// :199  the trial is rejected.  Written so that a NaN merit is accepted, as the scripts' `while cF_new > ...` does.
static inline bool apd_armijo_rejects(double cF_new, double cF_old, double nu, double step, double ress) {
    return cF_new > cF_old - nu * step * ress;
}

static inline double apd_trial_step(double delta, int ll) { return std::pow(delta, (double)ll); }

// A rejected first trial is followed by dozens more (delta = 0.9): they are taken MK per pass, on the merit alone,
// unless the merit needs the sums only the full evaluation makes (prob 3) or no further trial is allowed.
static inline bool apd_ls_batched(bool first_rejected, bool merit3, int ll_max) {
    return first_rejected && !merit3 && ll_max > 0;
}

// the steps of the batch that follows `ll` rejected trials: delta^(ll+1+k), k < MK
static inline void apd_batch_steps(double delta, int ll, double st[MK]) {
    for (int k = 0; k < MK; ++k) st[k] = apd_trial_step(delta, ll + 1 + k);
}

// The first trial of the batch that the sequential rule would stop at: the Armijo test holds, or it is trial ll_max.
// Found: *ll is that trial.  Not found: *ll moves past the batch (the clamp below undoes an overshoot of ll_max).
static inline bool apd_batch_pick(const double mv[MK], const double st[MK], double cF_old, double nu, double ress,
                                  int ll_max, int* ll) {
    for (int k = 0; k < MK; ++k) {
        const int cand = *ll + 1 + k;
        if (cand > ll_max) break;
        if (!apd_armijo_rejects(mv[k], cF_old, nu, st[k], ress) || cand == ll_max) {
            *ll = cand;
            return true;
        }
    }
    *ll += MK;
    return false;
}

static inline int apd_ls_clamp(int ll, int ll_max) { return std::min(ll, ll_max); }

// ---------------------------------------------------------------------------
// the SsN loop's stop tests                                                      :137,213-226
// ---------------------------------------------------------------------------
static inline bool apd_ssn_wants_step(double normF, double ssn_tol) { return normF > ssn_tol; }      // :137
static inline bool apd_ssn_solved(double normF_new, double ssn_tol) { return normF_new <= ssn_tol; } // :213
static inline bool apd_ssn_stalled(bool cls2, double normF_old, double normF_new, double ssn_tol) {  // :219
    return std::fabs(normF_old - normF_new) < apd_stall_bound(cls2, ssn_tol);
}
static inline bool apd_ssn_exhausted(int ssn_it, int ssn_it_max) { return ssn_it == ssn_it_max; }    // :226

// ---------------------------------------------------------------------------
// acceptance of a step                                                           :239-254
// ---------------------------------------------------------------------------
// kk, kkt0: KKT_xk, KKT_lk, KKT_yk, KKT_zk (the last two are class 2's)
static inline double apd_resk(bool cls2, const double kk[4]) {
    double r = std::max(kk[0], kk[1]);
    if (cls2) r = std::max(std::max(r, kk[2]), kk[3]);
    return r;
}

static inline double apd_max_rr(bool cls2, const double kk[4], const double kkt0[4]) {
    double r = std::max(kk[0] / (1.0 + kkt0[0]), kk[1] / (1.0 + kkt0[1]));
    if (cls2) {
        r = std::max(r, kk[2] / (1.0 + kkt0[2]));
        r = std::max(r, kk[3] / (1.0 + kkt0[3]));
    }
    return r;
}

static inline bool apd_restarts(double bk1, double rr, double resk) { return bk1 < 1e-8 && rr > resk; }   // :245

static inline double apd_restart_bk_class2(double bk1) { return 10.0 * bk1; }                 // Class2 :255

// ---------------------------------------------------------------------------
// the stopping rule on the certified gap (ipd_apd_set_gap_rule)
// ---------------------------------------------------------------------------
// a probe follows iteration k: at first, first + every, ... and at the iteration that converged
static inline bool apd_gap_due(int k, int first, int every, bool converged) {
    return converged || (k >= first && (k - first) % every == 0);
}

// the better of the two repaired multipliers: the larger dual value, side 0 on a tie and against a NaN
// (APDWorkspace.certificate's `1 if d1 > d0 else 0`)
static inline int apd_gap_lower_side(double dual0, double dual1) { return dual1 > dual0 ? 1 : 0; }

// the better of the two rounded plans: a repaired one first, then the smaller cost, side 0 on a tie and against a NaN
// (APDWorkspace.bracket's `min((0, 1), key=lambda s: (not ok[s], fval[s]))`)
static inline int apd_gap_upper_side(int ok0, double fval0, int ok1, double fval1) {
    return (ok1 > ok0 || (ok1 == ok0 && fval1 < fval0)) ? 1 : 0;
}

// every probe's dual value bounds f* from below, whatever the iterate: the best one so far stays (a NaN never enters)
static inline bool apd_gap_improves(double lower, double best) { return lower > best; }
static inline double apd_gap_best(double lower, double best) { return apd_gap_improves(lower, best) ? lower : best; }

static inline double apd_gap_value(double upper, double best) { return upper - best; }

// thr = max(gap_tol, gap_rel*|upper|); 0: the rule records and never stops
static inline double apd_gap_threshold(double gap_tol, double gap_rel, double upper) {
    const double rel = gap_rel * std::fabs(upper);
    return rel > gap_tol ? rel : gap_tol;   // a NaN upper leaves gap_tol
}

// a NaN gap never stops
static inline bool apd_gap_stops(double thr, int upper_ok, double gap) {
    return thr > 0.0 && upper_ok != 0 && gap <= thr;
}

// ---------------------------------------------------------------------------
// routes
// ---------------------------------------------------------------------------
// how zeta = Jk \ (-Fk_old) is found                        :146-161 / Class2 :152-171
enum ApdRoute {
    ROUTE_DIRECT,       // 1, class 1: build Jk, sparse Cholesky
    ROUTE_DIRECT_POT,   // 1, class 2: the bordered system, direct
    ROUTE_PCG,          // 2, class 1: PCG(Jk, -Fk_old)
    ROUTE_PCG_POT,      // 2, class 2: PCG on the bordered Jk
    ROUTE_AUG_PCG,      // 3, class 1
    ROUTE_PCG4POT,      // 3, class 2
    ROUTE_HYBRID_AMG,   // 4 'amg', 5 'twogrid', class 1
    ROUTE_AMG4POT       // 4, 5, class 2
};

static inline ApdRoute apd_route(bool cls2, int inner_solver) {
    switch (inner_solver) {
        case 1: return cls2 ? ROUTE_DIRECT_POT : ROUTE_DIRECT;
        case 2: return cls2 ? ROUTE_PCG_POT : ROUTE_PCG;
        case 3: return cls2 ? ROUTE_PCG4POT : ROUTE_AUG_PCG;
        default: return cls2 ? ROUTE_AMG4POT : ROUTE_HYBRID_AMG;
    }
}

// which instantiation of the evaluation pass runs (OpEvalT<CLS2, GVEC, M3>): class 2 has one
enum ApdEvalKind { EVAL_CLS2, EVAL_GVEC_M3, EVAL_GVEC, EVAL_GS_M3, EVAL_GS };

static inline ApdEvalKind apd_eval_kind(bool cls2, bool gama_vector, bool merit3) {
    if (cls2) return EVAL_CLS2;
    if (gama_vector) return merit3 ? EVAL_GVEC_M3 : EVAL_GVEC;
    return merit3 ? EVAL_GS_M3 : EVAL_GS;
}

// algorithmic bytes of one evaluation pass: wk read + mask written (+ phi, + gama when they are vectors), the
// multiplier/p/q vectors and the partial sums
static inline double apd_eval_bytes(const Geo& g, bool have_phi, bool have_gama) {
    const double mn = (double)((size_t)g.m * g.n);
    double by = 8.0 * mn + mn + 16.0 * (g.m + g.n);
    if (have_phi) by += 8.0 * mn;
    if (have_gama) by += 8.0 * mn;
    by += 8.0 * ((double)g.njg * g.m + 4.0 * g.nib * g.n);
    return by;
}
