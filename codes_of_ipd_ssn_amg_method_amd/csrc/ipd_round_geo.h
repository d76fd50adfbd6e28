// Geometry of the primal certificate of ipd_round.hip: the scalars of the walking passes and
// the scratch a call takes, on the column-group walk of ipd_walk_geo.h, whose row and column partials (walk_row_part_*,
// walk_col_part_*) the passes write as they stand.  Host-clean: no HIP types, no getenv (the index functions are
// __host__ __device__ under hipcc only) -- the CPU test of this header (tests/round_geo_driver.cpp) checks what the
// device runs.
//
//   scalars       RD_NS sums per workgroup, workgroup (ib, grp) at walk_block_index*RD_NS
// The finishing kernels combine the partials of a row or a column in index order; the last kernel combines the
// workgroups' scalars (thread t adds workgroups t, t + 256, ... in order, then a fixed tree).  The row and the
// column buffer are one pair for all passes: a pass's partials are combined before the next pass writes them.
#pragma once

#include <cstdint>

#include "ipd_walk_geo.h"

constexpr int RD_NS = 2;    // scalar sums a walking pass leaves per workgroup
constexpr int RD_NVEC = 4;  // vectors of n + m entries a call keeps: [b0; a0], [kappa; rho], [b2; a2], [f; e]
constexpr int RD_RESULT_DOUBLES = 24;   // the statistics and the scalars the device keeps for the writing pass

using RdGeo = WalkGeo;

WK_HD_INLINE size_t rd_scal_index(const RdGeo& g, int ib, int grp, int k) {
    return walk_block_index<size_t>(g, ib, grp) * RD_NS + (size_t)k;
}
WK_HD_INLINE size_t rd_scal_len(const RdGeo& g) { return (size_t)walk_blocks(g) * RD_NS; }
constexpr int RD_SCAL_PASSES = 3;   // passes A, C and D each keep their scalars until the last kernel

// bytes a call takes from the scratch arena (allocation granules of the arena aside): the two partial buffers, the
// scalars of three passes, the vectors and the result.  Nothing here depends on the class, the side or the entry:
// the host entry reads the vectors it returns out of the same scratch.
static inline size_t round_scratch_bytes(const RdGeo& g) {
    const size_t M = (size_t)g.m + (size_t)g.n;
    return (walk_row_part_len(g) + walk_col_part_len(g) + RD_SCAL_PASSES * rd_scal_len(g) + RD_NVEC * M +
            RD_RESULT_DOUBLES) * sizeof(double);
}
