// Geometry of the plan products Y = X*B (side 0) and Y = X'*B (side 1) of ipd_plan_apply.hip: the split of B's k
// columns into passes and the sizes and indexing of the partial buffer, on the column-group walk of ipd_walk_geo.h.
// The launcher, both walking kernels and the finishing kernel take every index from here.  Host-clean: no HIP types, no
// getenv (the index functions are __host__ __device__ under hipcc only) -- the CPU test of this header
// (tests/plan_apply_geo_driver.cpp) checks what the device runs.
//
// B's columns ("components") go PA_KC at a time: pass p takes the components [p*PA_KC, p*PA_KC + pa_pass_kc(g, p)),
// one launch of the walker and one of the finishing kernel per pass, and x is read once per pass.  The mass w = X*1
// (X'*1) is component PA_KC of pass 0.
//
// The partial buffer is the passes' in turn (launches on one stream), so it holds PA_NC = PA_KC + 1 components:
//   side 0   a lane's row sums over its column group:            S = ng    partials per entry of Y, R = m rows out
//   side 1   a wave's column sums over its 64 rows (a segment):  S = nslot partials per entry of Y, R = n rows out
//   entry (s, comp, r) at ((s * PA_NC + comp) * R + r); the finishing kernel adds s = 0 .. S-1 in that order.
// That is 8 * PA_NC * S * R bytes, about 0.625 * mn whatever k is (why the groups are WK_CPG chunks wide:
// ipd_walk_geo.h).  A call's whole scratch (pa_scratch_bytes) adds the mass when the caller passes no w (8 * R) and,
// for the host entry, the device copies of B, Y and w (8 * (k*(m+n) + R)); allocation granules of the arena aside.
// From m = n = 1024 on this is below 2*mn bytes, a quarter of one mn vector (the test walks the shapes).
#pragma once

#include "ipd_walk_geo.h"

constexpr int PA_KMAX = 16;         // columns of B
constexpr int PA_KC = 4;            // components per pass
constexpr int PA_NC = PA_KC + 1;    // components of the partial buffer: a pass's columns and the mass

struct PaOwn {
    int k, side;
};
struct PaGeo : WalkGeoT<PaOwn> {
    int npass;   // passes over x
};

static inline PaGeo pa_make_geo(int m, int n, int k, int side) {
    PaGeo g;
    static_cast<WalkGeoT<PaOwn>&>(g) = walk_make_geo(m, n, PaOwn{k, side});
    g.npass = apd_cdiv(k, PA_KC);
    return g;
}

// pass p: first component and number of components (PA_KC, the last pass k mod PA_KC when that is not 0)
WK_HD_INLINE int pa_pass_c0(int p) { return p * PA_KC; }
static inline int pa_pass_kc(const PaGeo& g, int p) {
    const int left = g.own.k - p * PA_KC;
    return left < PA_KC ? left : PA_KC;
}

WK_HD_INLINE int pa_out_rows(const PaGeo& g) { return g.own.side ? g.n : g.m; }      // R
WK_HD_INLINE int pa_part_count(const PaGeo& g) { return g.own.side ? g.nslot : g.ng; }   // S
WK_HD_INLINE size_t pa_part_stride(const PaGeo& g) { return (size_t)PA_NC * (size_t)pa_out_rows(g); }
WK_HD_INLINE size_t pa_part_index(const PaGeo& g, int s, int comp, int r) {
    return ((size_t)s * PA_NC + (size_t)comp) * (size_t)pa_out_rows(g) + (size_t)r;
}
WK_HD_INLINE size_t pa_part_len(const PaGeo& g) { return (size_t)pa_part_count(g) * pa_part_stride(g); }

// bytes a call takes from the scratch arena: own_mass = the caller gave no w but normalize needs one; host_entry =
// ipd_apd_plan_apply (device copies of B and Y, and of w when the caller wants it)
static inline size_t pa_scratch_bytes(const PaGeo& g, bool own_mass, bool host_entry, bool host_w) {
    size_t d = pa_part_len(g);
    if (own_mass) d += (size_t)pa_out_rows(g);
    if (host_entry) {
        d += (size_t)g.own.k * ((size_t)g.m + (size_t)g.n);
        if (host_w) d += (size_t)pa_out_rows(g);
    }
    return d * sizeof(double);
}
