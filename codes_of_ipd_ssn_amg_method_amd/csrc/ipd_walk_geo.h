// The column-group walk of the plan products (ipd_plan_apply.hip), the dual certificate (ipd_dual.hip) and the primal
// certificate (ipd_round.hip), stated once: the column-group rule, the grid, the segment slots
// and the two strided partial layouts.  The units' own headers (ipd_plan_apply_geo.h, ipd_dual_geo.h,
// ipd_round_geo.h) add what is theirs; the kernels' frame on top of it is ipd_walk_dev.h.  Host-clean: no HIP types, no
// getenv (the index functions are __host__ __device__ under hipcc only) -- the CPU test of this header
// (tests/walk_geo_driver.cpp) checks what the device runs.
//
// x(i,j) = x[i + j*m].  A workgroup is APD_WAVES waves of 64 consecutive rows each (TR rows, the tile walker's), a
// wave walks WK_CPG chunks of TC columns alone: the grid is nib x ng, workgroup (ib, grp) has the index
// walk_block_index, and column group `grp` owns the columns [grp*WK_CPG*TC, (grp+1)*WK_CPG*TC) below n.  Wave `wv` of
// row block `ib` is the segment slot walk_slot(ib, wv), of a segment without rows too.  What a walk leaves behind:
//   per row      a lane's result over its column group:            ng    partials per row,    (grp, i)  at grp*m + i
//   per column   a wave's result over its 64 rows (a segment):     nslot partials per column, (slot, j) at slot*n + j
//   per group    one record per workgroup at walk_block_index
// and a finishing kernel combines the partials of a row, a column or the workgroups in index order.
//
// Why WK_CPG = 4.  The tile walker's one chunk per group would leave n/16 partial rows per component of the plan
// products: at k = 16, all components kept, that is as large as x itself.  With groups of WK_CPG*TC = 64 columns a
// partial stands for 64 entries of x on either side (per column: the 64 rows of a wave), so that buffer is
//   8 * PA_NC * S * R  bytes  =  8 * 5 * ceil(n/64) * m  (per row)   or   8 * 5 * 4*ceil(m/256) * n  (per column),
// about 0.625 * mn -- whatever k is, since the passes share it (ipd_plan_apply_geo.h).  Wider groups would shrink it
// further but leave nib * ng = 1024 workgroups at m = n = 4096 already; narrower ones are not needed for the suite:
// (65, 150) has three groups with a partly filled last one.
#pragma once

#include "ipd_apd_geo.h"

#if defined(__HIPCC__)
#define WK_HD_INLINE __host__ __device__ __forceinline__   // the kernels index with these functions too
#else
#define WK_HD_INLINE static inline
#endif

constexpr int WK_CPG = 4;   // chunks of TC columns per column group

// The walk of an m x n array.  A unit's own numbers (Own: the side, the number of components) stand between the shape
// and the grid, where its kernels have always read them: the geometry is the head of every kernel's argument block,
// and a field that moved would be another kernel.
struct WalkNoOwn {};
template <class Own>
struct WalkGeoT {
    int m, n;
    [[no_unique_address]] Own own;
    int nib, ng, nslot;   // grid nib x ng; nslot = APD_WAVES * nib segment slots
};
using WalkGeo = WalkGeoT<WalkNoOwn>;

template <class Own = WalkNoOwn>
static inline WalkGeoT<Own> walk_make_geo(int m, int n, Own own = Own()) {
    WalkGeoT<Own> g;
    g.m = m;
    g.n = n;
    g.own = own;
    g.nib = apd_cdiv(m, TR);
    g.ng = apd_cdiv(apd_cdiv(n, TC), WK_CPG);
    g.nslot = APD_WAVES * g.nib;
    return g;
}

// first column of chunk `ch` of column group `grp`; the chunk owns columns [j0, j0 + TC) below n and the group's walk
// ends when j0 >= n
WK_HD_INLINE int walk_chunk_col(int grp, int ch) { return (grp * WK_CPG + ch) * TC; }
// the segment slot of wave `wv` of row block `ib`
WK_HD_INLINE int walk_slot(int ib, int wv) { return ib * APD_WAVES + wv; }

template <class Own>
WK_HD_INLINE int walk_blocks(const WalkGeoT<Own>& g) { return g.nib * g.ng; }
// (in the width the caller indexes with)
template <class I = int, class Own>
WK_HD_INLINE I walk_block_index(const WalkGeoT<Own>& g, int ib, int grp) { return (I)grp * (I)g.nib + (I)ib; }

template <class Own>
WK_HD_INLINE size_t walk_row_part_index(const WalkGeoT<Own>& g, int grp, int i) { return (size_t)grp * (size_t)g.m + (size_t)i; }
template <class Own>
WK_HD_INLINE size_t walk_row_part_len(const WalkGeoT<Own>& g) { return (size_t)g.ng * (size_t)g.m; }
template <class Own>
WK_HD_INLINE size_t walk_col_part_index(const WalkGeoT<Own>& g, int slot, int j) { return (size_t)slot * (size_t)g.n + (size_t)j; }
template <class Own>
WK_HD_INLINE size_t walk_col_part_len(const WalkGeoT<Own>& g) { return (size_t)g.nslot * (size_t)g.n; }
