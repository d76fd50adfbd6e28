// Geometry of the primal certificate of ipd_round.hip: the column-group rule, the grid, the
// sizes and indexing of the partial buffers of the walking passes, and the scratch a call takes.  The launcher, the
// walking kernels and the finishing kernels take every index from here.  Host-clean: no HIP types, no getenv (the
// index functions are __host__ __device__ under hipcc only) -- the CPU test of this header
// (tests/round_geo_driver.cpp) checks what the device runs.
//
// x(i,j) = x[i + j*m].  A workgroup is APD_WAVES waves of 64 consecutive rows each (TR rows, the tile walker's), a
// wave walks RD_CPG chunks of TC columns alone: the grid is nib x ng, and column group `grp` owns the columns
// [grp*RD_CPG*TC, (grp+1)*RD_CPG*TC) below n -- the walk of ipd_dual_geo.h, so a partial stands for 64 entries of x
// on either side.
//
//   row sums      a lane's sum over its column group:           ng    partials per row,    entry (grp, i)  at grp*m + i
//   column sums   a wave's sum over its 64 rows (a segment):    nslot partials per column, entry (slot, j) at slot*n+j
//                 (slot = ib*APD_WAVES + wave; colsum16's butterfly, ipd_apd_tiles.h)
//   scalars       RD_NS sums per workgroup, workgroup (ib, grp) at (grp*nib + ib)*RD_NS
// The finishing kernels combine the partials of a row or a column in index order; the last kernel combines the
// workgroups' scalars (thread t adds workgroups t, t + 256, ... in order, then a fixed tree).  The row and the
// column buffer are one pair for all passes: a pass's partials are combined before the next pass writes them.
#pragma once

#include <cstdint>

#include "ipd_apd_geo.h"

#if defined(__HIPCC__)
#define RD_HD_INLINE __host__ __device__ __forceinline__   // the kernels index with these functions too
#else
#define RD_HD_INLINE static inline
#endif

constexpr int RD_CPG = 4;   // chunks of TC columns per column group
constexpr int RD_NS = 2;    // scalar sums a walking pass leaves per workgroup
constexpr int RD_NVEC = 4;  // vectors of n + m entries a call keeps: [b0; a0], [kappa; rho], [b2; a2], [f; e]
constexpr int RD_RESULT_DOUBLES = 24;   // the statistics and the scalars the device keeps for the writing pass

struct RdGeo {
    int m, n;
    int nib, ng, nslot;      // grid nib x ng; nslot = APD_WAVES * nib segment slots
};

static inline RdGeo rd_make_geo(int m, int n) {
    RdGeo g;
    g.m = m;
    g.n = n;
    g.nib = apd_cdiv(m, TR);
    g.ng = apd_cdiv(apd_cdiv(n, TC), RD_CPG);
    g.nslot = APD_WAVES * g.nib;
    return g;
}

// first column of chunk `ch` of column group `grp`; the chunk owns columns [j0, j0 + TC) below n and the group's walk
// ends when j0 >= n
RD_HD_INLINE int rd_chunk_col(int grp, int ch) { return (grp * RD_CPG + ch) * TC; }
// the segment slot of wave `wv` of row block `ib`
RD_HD_INLINE int rd_slot(int ib, int wv) { return ib * APD_WAVES + wv; }

RD_HD_INLINE size_t rd_row_index(const RdGeo& g, int grp, int i) { return (size_t)grp * (size_t)g.m + (size_t)i; }
RD_HD_INLINE size_t rd_row_len(const RdGeo& g) { return (size_t)g.ng * (size_t)g.m; }
RD_HD_INLINE size_t rd_col_index(const RdGeo& g, int slot, int j) { return (size_t)slot * (size_t)g.n + (size_t)j; }
RD_HD_INLINE size_t rd_col_len(const RdGeo& g) { return (size_t)g.nslot * (size_t)g.n; }

RD_HD_INLINE int rd_blocks(const RdGeo& g) { return g.nib * g.ng; }
RD_HD_INLINE size_t rd_scal_index(const RdGeo& g, int ib, int grp, int k) {
    return ((size_t)grp * (size_t)g.nib + (size_t)ib) * RD_NS + (size_t)k;
}
RD_HD_INLINE size_t rd_scal_len(const RdGeo& g) { return (size_t)rd_blocks(g) * RD_NS; }
constexpr int RD_SCAL_PASSES = 3;   // passes A, C and D each keep their scalars until the last kernel

// bytes a call takes from the scratch arena (allocation granules of the arena aside): the two partial buffers, the
// scalars of three passes, the vectors and the result.  Nothing here depends on the class, the side or the entry:
// the host entry reads the vectors it returns out of the same scratch.
static inline size_t round_scratch_bytes(const RdGeo& g) {
    const size_t M = (size_t)g.m + (size_t)g.n;
    return (rd_row_len(g) + rd_col_len(g) + RD_SCAL_PASSES * rd_scal_len(g) + RD_NVEC * M + RD_RESULT_DOUBLES) *
           sizeof(double);
}
