// The gradient of the transport cost in the point positions (ipd_point_grad.hip): one weight
// dc/dx restated as scalar code, the split of the d output components into passes and the sizes and indexing of the
// partial buffers, on the column-group walk of ipd_walk_geo.h.  The kernels fold a pair and form a weight with the
// functions below and take every index from here, so that the CPU test of this header
// (tests/point_grad_geo_driver.cpp) checks what the device runs.  Host-clean: no HIP types, no getenv.
//
// With X the plan at the threshold tol (x(i,j) = u[i + j*m], kept when !(|x| <= tol)) and c the cost of two point
// clouds (ipd_cost_plan.h), the envelope theorem gives at an optimal or rounded feasible X
//   side 0   G(i,k) = sum_j X_ij * h_k(i,j)        h_k = dc(xs_i, ys_j) / dxs(i,k)
//   side 1   G(j,k) = sum_i X_ij * (-h_k(i,j))     dc / dys(j,k) = -h_k
// With t_k = xs(i,k) - ys(j,k) (the subtraction of cost_fold), every step one IEEE operation:
//   1 sq. Euclidean   h_k = t_k + t_k
//   2 Euclidean       a = sqrt(sum t_k*t_k) folded as cost_fold<2> / cost_finish<2> in ascending k;
//                     h_k = t_k / a when a > 0, else +0.0 (a select: no 0/0 is formed)
//   3 city block      h_k = +1.0, -1.0 or +0.0 by the sign of t_k
//   4 Chebyshev       k* = the smallest k with |t_k| equal to the fold's maximum (strict > while folding in ascending
//                     k); h_k* = the sign of t_k* as in metric 3, every other h_k = +0.0
// Where c is not differentiable (a kink: metric 2 a == 0; metric 3 some t_k == 0; metric 4 the maximum attained by two
// coordinates, or 0) this is one element of the subdifferential, and the kept entries there are counted.  scale = 1
// divides h_k by the largest unscaled entry, one division applied last: the normalisation is held constant (a
// stop-gradient), the divider is handed back so that a caller can add the missing term.
//
// Output components go PG_KC at a time: pass p takes the components [p*PG_KC, p*PG_KC + pg_pass_kc(g, p)), one launch
// of the walker and one of the finishing kernel per pass.  d <= PG_DT_MAX runs as one pass with the row coordinates in
// registers, larger d with the workgroup's row coordinates in LDS ([k][thread], 8 * 16 * 256 bytes).  The mass
// w = X*1 (X'*1) is component PG_KC of pass 0.  The partial buffer is the passes' in turn and holds PG_NC planes:
//   side 0   plane comp, (grp, i)  at comp*S*R + walk_row_part_index   S = ng,    R = m
//   side 1   plane comp, (slot, j) at comp*S*R + walk_col_part_index   S = nslot, R = n
// the finishing kernel adds s = 0 .. S-1 in that order at stride R.  Beside it one record of PG_REC 64-bit counts per
// workgroup at walk_block_index: the kept entries and the kept entries at a kink.
#pragma once

#include <cstdint>

#include "ipd_cost_plan.h"
#include "ipd_walk_geo.h"

constexpr int PG_KC = 4;            // components per pass
constexpr int PG_NC = PG_KC + 1;    // planes of the partial buffer: a pass's components and the mass
constexpr int PG_DT_MAX = COST_DT_MAX;   // dimensions up to which the row coordinates are template registers
constexpr int PG_REC = 2;           // counts per workgroup: kept, kinks
constexpr int PG_STATS_DOUBLES = 3; // doubles a device copy of ipd_grad_stats takes
static_assert(PG_DT_MAX <= PG_KC, "the register form is one pass");

struct PgOwn {
    int d, side;
};
struct PgGeo : WalkGeoT<PgOwn> {
    int npass;   // passes over x
};

static inline PgGeo pg_make_geo(int m, int n, int d, int side) {
    PgGeo g;
    static_cast<WalkGeoT<PgOwn>&>(g) = walk_make_geo(m, n, PgOwn{d, side});
    g.npass = apd_cdiv(d, PG_KC);
    return g;
}

// pass p: first component and number of components (PG_KC, the last pass d mod PG_KC when that is not 0)
WK_HD_INLINE int pg_pass_c0(int p) { return p * PG_KC; }
static inline int pg_pass_kc(const PgGeo& g, int p) {
    const int left = g.own.d - p * PG_KC;
    return left < PG_KC ? left : PG_KC;
}
// how often x is read: once for d <= PG_KC, ceil(d / PG_KC) times beyond
static inline int pg_x_reads(const PgGeo& g) { return g.npass; }

WK_HD_INLINE int pg_out_rows(const PgGeo& g) { return g.own.side ? g.n : g.m; }        // R
WK_HD_INLINE int pg_part_count(const PgGeo& g) { return g.own.side ? g.nslot : g.ng; }   // S
WK_HD_INLINE size_t pg_part_stride(const PgGeo& g) { return (size_t)pg_out_rows(g); }
WK_HD_INLINE size_t pg_plane_len(const PgGeo& g) { return g.own.side ? walk_col_part_len(g) : walk_row_part_len(g); }
WK_HD_INLINE size_t pg_part_index(const PgGeo& g, int s, int comp, int r) {
    return (size_t)comp * pg_plane_len(g) + (g.own.side ? walk_col_part_index(g, s, r) : walk_row_part_index(g, s, r));
}
WK_HD_INLINE size_t pg_part_len(const PgGeo& g) { return (size_t)PG_NC * pg_plane_len(g); }
WK_HD_INLINE size_t pg_rec_len(const PgGeo& g) { return (size_t)PG_REC * (size_t)walk_blocks(g); }

// bytes a call takes from the scratch arena (allocation granules aside): host_entry = ipd_apd_point_grad (device
// copies of G and, when wanted, of w); own_points = false: the (m+n)*d coordinates of a given specification go up too
static inline size_t pg_scratch_bytes(const PgGeo& g, bool host_entry, bool host_w, bool own_points) {
    size_t d = pg_part_len(g) + pg_rec_len(g) + (size_t)PG_STATS_DOUBLES;
    if (host_entry) {
        d += (size_t)g.own.d * (size_t)pg_out_rows(g);
        if (host_w) d += (size_t)pg_out_rows(g);
        if (!own_points) d += (size_t)g.own.d * ((size_t)g.m + (size_t)g.n);
    }
    return d * sizeof(double);
}

// ---------------------------------------------------------------------------------------------------------------
// One pair (i, j).  Its coordinates are folded in ascending k into a PgPair that starts at pg_pair_init(), finished
// once, and then give the weights h_k.  The compiler drops the fields a metric does not use.
// ---------------------------------------------------------------------------------------------------------------
struct PgPair {
    double acc;   // 2: sum t*t, after pg_pair_finish its root a;  4: max |t|
    int kstar;    // 4: the smallest k that attains the maximum
};
// The flag of a pair -- 3: some t_k == 0;  4: a later k attains the maximum too, or |t_0| == 0 -- is bit `bit` of a
// word that the caller keeps for the pairs it folds together (the 16 columns of a chunk; one pair: bit 0).  As lane
// masks the 16 flags would hold scalar registers the kernels cannot spare.

IPD_HD_INLINE PgPair pg_pair_init() {
    PgPair f;
    f.acc = 0.0;
    f.kstar = 0;
    return f;
}

template <int METRIC>
IPD_HD_INLINE void pg_pair_fold(PgPair& f, unsigned& flags, int bit, int k, double x, double y) {
    const unsigned b = 1u << bit;
    if (METRIC == COST_EUCLIDEAN) {
        f.acc = cost_fold<COST_EUCLIDEAN>(f.acc, x, y);
    } else if (METRIC == COST_CITYBLOCK) {
        const double t = x - y;
        flags |= t == 0.0 ? b : 0u;
    } else if (METRIC == COST_CHEBYSHEV) {
        const double at = fabs(x - y);
        const bool up = at > f.acc;
        flags = up ? flags & ~b : (at == f.acc ? flags | b : flags);
        f.kstar = up ? k : f.kstar;
        f.acc = up ? at : f.acc;
    }
}
template <int METRIC>
IPD_HD_INLINE void pg_pair_finish(PgPair& f) {
    if (METRIC == COST_EUCLIDEAN) f.acc = cost_finish<COST_EUCLIDEAN>(f.acc);
}
// is c not differentiable at the (finished) pair?
template <int METRIC>
IPD_HD_INLINE bool pg_pair_kink(const PgPair& f, unsigned flags, int bit) {
    const bool flag = (flags >> bit & 1u) != 0;
    if (METRIC == COST_EUCLIDEAN) return f.acc == 0.0;
    if (METRIC == COST_CITYBLOCK) return flag;
    if (METRIC == COST_CHEBYSHEV) return flag || f.acc == 0.0;
    return false;
}
// does a metric's weight need the fold of all d coordinates (2, 4), or only its kink count (3)?
constexpr bool pg_needs_fold(int metric) { return metric == COST_EUCLIDEAN || metric == COST_CHEBYSHEV; }

IPD_HD_INLINE double pg_sign(double t) { return t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : 0.0); }

// h_k of the finished pair, unscaled
template <int METRIC>
IPD_HD_INLINE double pg_h(const PgPair& f, int k, double x, double y) {
    const double t = x - y;
    if (METRIC == COST_SQEUCLIDEAN) return t + t;
    if (METRIC == COST_EUCLIDEAN) {
        const bool pos = f.acc > 0.0;
        const double q = t / (pos ? f.acc : 1.0);
        return pos ? q : 0.0;
    }
    if (METRIC == COST_CITYBLOCK) return pg_sign(t);
    return k == f.kstar ? pg_sign(t) : 0.0;
}
// scale = 1: one division, applied last
IPD_HD_INLINE double pg_scaled(double h, int divide, double denom) { return divide ? h / denom : h; }
// what a kept entry adds: x*h_k on side 0, x*(-h_k) on side 1, the negation exact
IPD_HD_INLINE double pg_term(double x, double h, int side) { return x * (side ? -h : h); }

// the restatement of one weight from the d coordinates of the two points (contiguous), for the CPU test
template <int METRIC>
static inline double pg_weight_of(int d, const double* xi, const double* yj, int k, int divide, double denom, int side,
                                  int* kink) {
    PgPair f = pg_pair_init();
    unsigned flags = 0;
    for (int kk = 0; kk < d; ++kk) pg_pair_fold<METRIC>(f, flags, 0, kk, xi[kk], yj[kk]);
    pg_pair_finish<METRIC>(f);
    if (kink) *kink = pg_pair_kink<METRIC>(f, flags, 0) ? 1 : 0;
    const double h = pg_scaled(pg_h<METRIC>(f, k, xi[k], yj[k]), divide, denom);
    return side ? -h : h;
}
static inline double pg_weight(int metric, int d, const double* xi, const double* yj, int k, int divide, double denom,
                               int side, int* kink) {
    switch (metric) {
        case COST_SQEUCLIDEAN: return pg_weight_of<COST_SQEUCLIDEAN>(d, xi, yj, k, divide, denom, side, kink);
        case COST_EUCLIDEAN: return pg_weight_of<COST_EUCLIDEAN>(d, xi, yj, k, divide, denom, side, kink);
        case COST_CITYBLOCK: return pg_weight_of<COST_CITYBLOCK>(d, xi, yj, k, divide, denom, side, kink);
        default: return pg_weight_of<COST_CHEBYSHEV>(d, xi, yj, k, divide, denom, side, kink);
    }
}
