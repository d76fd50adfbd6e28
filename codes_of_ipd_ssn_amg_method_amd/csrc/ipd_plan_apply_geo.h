// Geometry of the plan products Y = X*B (side 0) and Y = X'*B (side 1) of ipd_plan_apply.hip: the column-group
// rule, the split of B's k columns into passes, the grid, and the sizes and indexing of the partial buffer.  The
// launcher, both walking kernels and the finishing kernel take every index from here.  Host-clean: no HIP types, no
// getenv (the index functions are __host__ __device__ under hipcc only) -- the CPU test of this header
// (tests/plan_apply_geo_driver.cpp) checks what the device runs.
//
// x(i,j) = x[i + j*m].  A workgroup is APD_WAVES waves of 64 consecutive rows each (TR rows, the tile walker's), a
// wave walks PA_CPG chunks of TC columns alone: the grid is nib x ng, and column group `grp` owns the columns
// [grp*PA_CPG*TC, (grp+1)*PA_CPG*TC) below n.  B's columns ("components") go PA_KC at a time: pass p takes the
// components [p*PA_KC, p*PA_KC + pa_pass_kc(g, p)), one launch of the walker and one of the finishing kernel per
// pass, and x is read once per pass.  The mass w = X*1 (X'*1) is component PA_KC of pass 0.
//
// The partial buffer is the passes' in turn (launches on one stream), so it holds PA_NC = PA_KC + 1 components:
//   side 0   a lane's row sums over its column group:            S = ng    partials per entry of Y, R = m rows out
//   side 1   a wave's column sums over its 64 rows (a segment):  S = nslot partials per entry of Y, R = n rows out
//   entry (s, comp, r) at ((s * PA_NC + comp) * R + r); the finishing kernel adds s = 0 .. S-1 in that order.
//
// Why PA_CPG = 4.  The tile walker's one chunk per group would leave n/16 partial rows per component: at k = 16, all
// components kept, that is as large as x itself.  With groups of PA_CPG*TC = 64 columns a partial stands for 64
// entries of x on either side (side 1: the 64 rows of a wave), so the buffer is
//   8 * PA_NC * S * R  bytes  =  8 * 5 * ceil(n/64) * m  (side 0)   or   8 * 5 * 4*ceil(m/256) * n  (side 1),
// about 0.625 * mn -- whatever k is, since the passes share it.  A call's whole scratch (pa_scratch_bytes) adds the
// mass when the caller passes no w (8 * R) and, for the host entry, the device copies of B, Y and w
// (8 * (k*(m+n) + R)); allocation granules of the arena aside.  From m = n = 1024 on this is below 2*mn bytes, a
// quarter of one mn vector (the test walks the shapes).  Wider groups would shrink it further but leave
// nib * ng = 1024 workgroups at m = n = 4096 already; narrower ones are not needed for the suite: (65, 150) has three
// groups with a partly filled last one.
#pragma once

#include "ipd_apd_geo.h"

#if defined(__HIPCC__)
#define PA_HD_INLINE __host__ __device__ __forceinline__   // the kernels index with these functions too
#else
#define PA_HD_INLINE static inline
#endif

constexpr int PA_KMAX = 16;         // columns of B
constexpr int PA_KC = 4;            // components per pass
constexpr int PA_NC = PA_KC + 1;    // components of the partial buffer: a pass's columns and the mass
constexpr int PA_CPG = 4;           // chunks of TC columns per column group

struct PaGeo {
    int m, n, k, side;
    int nib, ng, nslot, npass;   // grid nib x ng; nslot = APD_WAVES * nib segment slots; npass passes over x
};

static inline PaGeo pa_make_geo(int m, int n, int k, int side) {
    PaGeo g;
    g.m = m;
    g.n = n;
    g.k = k;
    g.side = side;
    g.nib = apd_cdiv(m, TR);
    g.ng = apd_cdiv(apd_cdiv(n, TC), PA_CPG);
    g.nslot = APD_WAVES * g.nib;
    g.npass = apd_cdiv(k, PA_KC);
    return g;
}

// pass p: first component and number of components (PA_KC, the last pass k mod PA_KC when that is not 0)
PA_HD_INLINE int pa_pass_c0(int p) { return p * PA_KC; }
static inline int pa_pass_kc(const PaGeo& g, int p) {
    const int left = g.k - p * PA_KC;
    return left < PA_KC ? left : PA_KC;
}

// first column of chunk `ch` of column group `grp`; the chunk owns columns [j0, j0 + TC) below n and the group's walk
// ends when j0 >= n
PA_HD_INLINE int pa_chunk_col(int grp, int ch) { return (grp * PA_CPG + ch) * TC; }

PA_HD_INLINE int pa_out_rows(const PaGeo& g) { return g.side ? g.n : g.m; }      // R
PA_HD_INLINE int pa_part_count(const PaGeo& g) { return g.side ? g.nslot : g.ng; }   // S
PA_HD_INLINE size_t pa_part_stride(const PaGeo& g) { return (size_t)PA_NC * (size_t)pa_out_rows(g); }
PA_HD_INLINE size_t pa_part_index(const PaGeo& g, int s, int comp, int r) {
    return ((size_t)s * PA_NC + (size_t)comp) * (size_t)pa_out_rows(g) + (size_t)r;
}
PA_HD_INLINE size_t pa_part_len(const PaGeo& g) { return (size_t)pa_part_count(g) * pa_part_stride(g); }

// bytes a call takes from the scratch arena: own_mass = the caller gave no w but normalize needs one; host_entry =
// ipd_apd_plan_apply (device copies of B and Y, and of w when the caller wants it)
static inline size_t pa_scratch_bytes(const PaGeo& g, bool own_mass, bool host_entry, bool host_w) {
    size_t d = pa_part_len(g);
    if (own_mass) d += (size_t)pa_out_rows(g);
    if (host_entry) {
        d += (size_t)g.k * ((size_t)g.m + (size_t)g.n);
        if (host_w) d += (size_t)pa_out_rows(g);
    }
    return d * sizeof(double);
}
