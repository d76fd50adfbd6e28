// The cost matrix out of two point clouds (ipd_cost.hip): what a cost specification must
// satisfy, which rows and columns a wave of the build kernel owns, and one entry restated as scalar code.  The
// kernels take their rows and columns from the functions below and fold an entry with cost_fold / cost_finish, so
// that the CPU test of this header (tests/cost_plan_driver.cpp) checks what the device runs.  Host-clean: no HIP
// types, no getenv.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstring>

#include "ipd_limits.h"

enum CostMetric { COST_SQEUCLIDEAN = 1, COST_EUCLIDEAN = 2, COST_CITYBLOCK = 3, COST_CHEBYSHEV = 4 };

// ---------------------------------------------------------------------------------------------------------------
// Validation.  Everything is checked on the host before a launch; the (m+n)*d coordinates are read once.
// COST_SHAPE is the drivers' size limit (IPD_E_LIMIT, as ipd_apd_create answers it), every other failure is
// IPD_E_ARG.
// ---------------------------------------------------------------------------------------------------------------
enum CostCheck { COST_OK, COST_NULL, COST_METRIC, COST_DIM, COST_SHAPE, COST_SCALE, COST_COORD };
static constexpr const char* COST_CHECK_NAMES[] = {"OK", "NULL", "METRIC", "DIM", "SHAPE", "SCALE", "COORD"};
static constexpr const char* COST_CHECK_TEXT[] = {
    "",
    "cost spec: xs or ys is NULL",
    "cost spec: metric must be 1 (sq. Euclidean), 2 (Euclidean), 3 (city block) or 4 (Chebyshev)",
    "cost spec: dim must be in [1, 16]",
    "cost spec: m, n must be in [1, 16384]",
    "cost spec: scale must be 0 or 1",
    "cost spec: a coordinate is not finite",
};
static_assert(IPD_COST_DIM_MAX == 16 && IPD_APD_SIDE_MAX == 16384, "the texts above name the limits");

static inline bool cost_all_finite(const double* v, size_t count) {
    for (size_t t = 0; t < count; ++t)
        if (!std::isfinite(v[t])) return false;
    return true;
}

static inline CostCheck cost_spec_check(int metric, int dim, long long m, long long n, const double* xs,
                                        const double* ys, int scale) {
    if (!xs || !ys) return COST_NULL;
    if (metric < COST_SQEUCLIDEAN || metric > COST_CHEBYSHEV) return COST_METRIC;
    if (dim < 1 || dim > IPD_COST_DIM_MAX) return COST_DIM;
    if (m < 1 || n < 1 || m > IPD_APD_SIDE_MAX || n > IPD_APD_SIDE_MAX) return COST_SHAPE;
    if (scale != 0 && scale != 1) return COST_SCALE;
    if (!cost_all_finite(xs, (size_t)m * dim) || !cost_all_finite(ys, (size_t)n * dim)) return COST_COORD;
    return COST_OK;
}

// scale = 1 divides by the largest entry: it has to be a positive finite number (all points equal: 0; an
// overflowing distance: inf)
static inline bool cost_scale_ok(double largest) { return std::isfinite(largest) && largest > 0.0; }

// ---------------------------------------------------------------------------------------------------------------
// One entry.  t_k = x_k - y_k folded into acc (which starts at +0.0) in ascending k, multiply and add separate
// (every unit is built with -ffp-contract=off, and so is the CPU driver).
// ---------------------------------------------------------------------------------------------------------------
template <int METRIC>
IPD_HD_INLINE double cost_fold(double acc, double x, double y) {
    const double t = x - y;
    if (METRIC == COST_CITYBLOCK) return acc + fabs(t);
    if (METRIC == COST_CHEBYSHEV) return fmax(acc, fabs(t));
    const double sq = t * t;
    return acc + sq;
}
template <int METRIC>
IPD_HD_INLINE double cost_finish(double acc) {
    return METRIC == COST_EUCLIDEAN ? sqrt(acc) : acc;
}

template <int METRIC>
static inline double cost_entry_of(int d, const double* xi, const double* yj) {
    double acc = 0.0;
    for (int k = 0; k < d; ++k) acc = cost_fold<METRIC>(acc, xi[k], yj[k]);
    return cost_finish<METRIC>(acc);
}
// xi, yj: the d coordinates of the two points, contiguous
static inline double cost_entry(int metric, int d, const double* xi, const double* yj) {
    switch (metric) {
        case COST_SQEUCLIDEAN: return cost_entry_of<COST_SQEUCLIDEAN>(d, xi, yj);
        case COST_EUCLIDEAN: return cost_entry_of<COST_EUCLIDEAN>(d, xi, yj);
        case COST_CITYBLOCK: return cost_entry_of<COST_CITYBLOCK>(d, xi, yj);
        default: return cost_entry_of<COST_CHEBYSHEV>(d, xi, yj);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Matrix-free cost: a workspace that keeps the (m+n)*d coordinates and no c.  The passes
// that read c(i,j) recompute it from a CostSrc: the row's coordinates sit in registers, the column's are
// wave-uniform, and cost_src_value folds them exactly as k_cost_build folds what it stores -- cost_fold in
// ascending k, cost_finish, then the one IEEE division of scale = 1 -- so a recomputed entry has the stored
// entry's bits.  The metric is a wave-uniform switch around cost_fold<METRIC>; D is a template parameter, no
// register array is indexed by a run-time k.
// ---------------------------------------------------------------------------------------------------------------
#if defined(__clang__)
#define COST_UNROLL _Pragma("unroll")   // D <= 3 iterations: every index below is a constant after unrolling
#else
#define COST_UNROLL
#endif

struct CostSrc {
    const double* xs;   // m*dim, xs[i + k*m]
    const double* ys;   // n*dim, ys[j + k*n]
    int m, n;
    int dim, metric;
    int divide;         // != 0: every entry is divided by denom
    double denom;
};

enum CostFreeCheck { COST_FREE_OK, COST_FREE_DIM };
static constexpr const char* COST_FREE_TEXT[] = {
    "",
    "matrix-free cost: dim must be in [1, 3] (the row coordinates are registers); larger dim needs a stored cost",
};
static constexpr int COST_FREE_DIM_MAX = 3;
static inline CostFreeCheck cost_free_check(int dim) {
    return dim >= 1 && dim <= COST_FREE_DIM_MAX ? COST_FREE_OK : COST_FREE_DIM;
}

template <int METRIC, int D>
IPD_HD_INLINE double cost_src_fold_of(const double (&x)[D], const double (&y)[D]) {
    double acc = 0.0;
    COST_UNROLL
    for (int k = 0; k < D; ++k) acc = cost_fold<METRIC>(acc, x[k], y[k]);
    return cost_finish<METRIC>(acc);
}
// x, y: the D coordinates of row i and column j
template <int D>
IPD_HD_INLINE double cost_src_value(const CostSrc& s, const double (&x)[D], const double (&y)[D]) {
    double v;
    switch (s.metric) {
        case COST_SQEUCLIDEAN: v = cost_src_fold_of<COST_SQEUCLIDEAN, D>(x, y); break;
        case COST_EUCLIDEAN: v = cost_src_fold_of<COST_EUCLIDEAN, D>(x, y); break;
        case COST_CITYBLOCK: v = cost_src_fold_of<COST_CITYBLOCK, D>(x, y); break;
        default: v = cost_src_fold_of<COST_CHEBYSHEV, D>(x, y); break;
    }
    if (s.divide) v = v / s.denom;   // as k_cost_build: one IEEE division, after the metric's last operation
    return v;
}
template <int D>
IPD_HD_INLINE void cost_src_row(const CostSrc& s, int i, double (&x)[D]) {
    COST_UNROLL
    for (int k = 0; k < D; ++k) x[k] = s.xs[(size_t)k * s.m + i];
}
template <int D>
IPD_HD_INLINE void cost_src_col(const CostSrc& s, int j, double (&y)[D]) {
    COST_UNROLL
    for (int k = 0; k < D; ++k) y[k] = s.ys[(size_t)k * s.n + j];
}
template <int D>
IPD_HD_INLINE double cost_src_entry_of(const CostSrc& s, int i, int j) {
    double x[D], y[D];
    cost_src_row<D>(s, i, x);
    cost_src_col<D>(s, j, y);
    return cost_src_value<D>(s, x, y);
}
// entry (i, j) of a source that passed cost_free_check
IPD_HD_INLINE double cost_src_entry(const CostSrc& s, int i, int j) {
    switch (s.dim) {
        case 1: return cost_src_entry_of<1>(s, i, j);
        case 2: return cost_src_entry_of<2>(s, i, j);
        default: return cost_src_entry_of<3>(s, i, j);
    }
}
static_assert(COST_FREE_DIM_MAX == 3, "cost_src_entry instantiates D = 1, 2, 3");

// ---------------------------------------------------------------------------------------------------------------
// Launch geometry: the walk of the plan kernels (ipd_plan.hip).  c(i,j) = c[i + j*m]; lanes along i; a wave owns
// 64*rpl consecutive rows (lane l: rows rpl*l .. rpl*l + rpl - 1 of them, one 8-byte or one 16-byte store per
// column) and walks COST_TC*reps columns alone; a workgroup is 4 waves, the grid nib x njg.
// ---------------------------------------------------------------------------------------------------------------
static constexpr int COST_TC = 16;      // columns a wave has in flight
static constexpr int COST_WAVES = 4;    // waves of a workgroup
static constexpr int COST_DT_MAX = 3;   // dimensions up to which the row coordinates are template registers
static_assert(COST_FREE_DIM_MAX == COST_DT_MAX, "matrix-free keeps the row coordinates where k_cost_build<D> does");

struct CostGeo {
    int m, n, rpl;          // rpl: rows per lane, 1 or 2
    int wrows, brows;       // rows of a wave / of a workgroup
    int nib, njg, reps;     // njg column groups of reps*COST_TC columns
};

static inline int cost_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

static inline CostGeo cost_geo(int m, int n, int rpl) {
    CostGeo g;
    g.m = m;
    g.n = n;
    g.rpl = rpl;
    g.wrows = 64 * rpl;
    g.brows = COST_WAVES * g.wrows;
    g.nib = cost_cdiv(m, g.brows);
    const int njb = cost_cdiv(n, COST_TC);
    int reps = 1;   // a wave walks more columns once the grid is large anyway (as plan_geo)
    while (reps < 8 && (long long)g.nib * cost_cdiv(njb, reps * 2) >= 4096) reps *= 2;
    g.reps = reps;
    g.njg = cost_cdiv(njb, reps);
    return g;
}

// first row of lane `lane` of wave `wv` of row block `ib`; the lane owns rows [r, r + rpl) below m
IPD_HD_INLINE int cost_lane_row(const CostGeo& g, int ib, int wv, int lane) {
    return ib * g.brows + wv * g.wrows + lane * g.rpl;
}
// columns of step `rep` of column group `jg`: [j0, j0 + COST_TC) below n; j0 >= n ends the walk
IPD_HD_INLINE int cost_step_col(const CostGeo& g, int jg, int rep) { return (jg * g.reps + rep) * COST_TC; }

// Two rows per lane need 16-byte aligned stores: an even m and a 16-byte aligned array; the generic form (d above
// COST_DT_MAX, row coordinates in LDS: 8 * 16 * 256 bytes per row of a lane) keeps one.  `store_switch` is the
// value of IPD_COST_STORE (nullptr: unset): "8" and "16" force a form where it is possible (measurement, tests).
static constexpr bool COST_STORE16_DEFAULT = true;   // measured, DESIGN.md 4g: 24.0 against 28.2 us at m = n = 4096
static inline int cost_rows_per_lane(int m, int d, bool aligned16, const char* store_switch) {
    if ((m & 1) || !aligned16 || d > COST_DT_MAX) return 1;
    if (store_switch && !std::strcmp(store_switch, "16")) return 2;
    if (store_switch && !std::strcmp(store_switch, "8")) return 1;
    return COST_STORE16_DEFAULT ? 2 : 1;
}
