// Geometry of the dual certificate of ipd_dual.hip: the sizes and indexing of the partial
// buffers of the c-transform and of the evaluation pass, on the column-group walk of ipd_walk_geo.h.  The launcher,
// the walking kernels and the finishing kernels take every index from here.  Host-clean: no HIP types, no getenv (the
// index functions are __host__ __device__ under hipcc only) -- the CPU test of this header
// (tests/dual_geo_driver.cpp) checks what the device runs.
//
//   transform, side 0   a lane's (max, arg max) over its column group:          S = ng    partials per row,    R = m
//   transform, side 1   a wave's (max, arg max) over its 64 rows (a segment):   S = nslot partials per column, R = n
//     a partial is a value (double) and an index (int32) in two arrays of du_part_len entries, entry (s, r) at
//     s*R + r; the finishing kernel combines s = 0 .. S-1 in that order.
//   evaluate            one DuEvalPart per workgroup at walk_block_index; the last kernel combines them in index
//                       order.
#pragma once

#include <cstdint>

#include "ipd_walk_geo.h"

struct DuOwn {
    int side;   // 0 or 1 for a transform; the evaluation ignores it
};
using DuGeo = WalkGeoT<DuOwn>;

// what a workgroup of the evaluation pass leaves behind
struct DuEvalPart {
    double dmin;             // smallest reduced cost of the workgroup's entries (+inf: none; a NaN never wins)
    double cap, fval;        // sum gama*max(0,-d), sum c*x
    long long idx, nneg;     // first column-major place i + j*m of dmin; entries with d < 0
};

static inline DuGeo du_make_geo(int m, int n, int side) { return walk_make_geo(m, n, DuOwn{side}); }

WK_HD_INLINE int du_out_rows(const DuGeo& g) { return g.own.side ? g.n : g.m; }          // R
WK_HD_INLINE int du_part_count(const DuGeo& g) { return g.own.side ? g.nslot : g.ng; }   // S
WK_HD_INLINE size_t du_part_stride(const DuGeo& g) { return (size_t)du_out_rows(g); }
WK_HD_INLINE size_t du_part_index(const DuGeo& g, int s, int r) { return (size_t)s * (size_t)du_out_rows(g) + (size_t)r; }
WK_HD_INLINE size_t du_part_len(const DuGeo& g) { return (size_t)du_part_count(g) * du_part_stride(g); }

// bytes a call takes from the scratch arena (allocation granules of the arena aside).  transform: side 0 or 1;
// own_out: the caller gave no lam_out, the repaired multiplier lives in scratch; host_entry = ipd_apd_dual: device
// copies of lam (when given), lam_out and arg (when wanted).
static inline size_t du_scratch_bytes(const DuGeo& g, int cls, bool transform, bool own_out, bool host_entry,
                                      bool host_lam, bool host_out, bool host_arg) {
    const size_t L = (size_t)g.m + (size_t)g.n + (cls == 2 ? 1 : 0);
    size_t b = (size_t)walk_blocks(g) * sizeof(DuEvalPart) + 16 * sizeof(double);   // partials and the result
    if (transform) {
        b += du_part_len(g) * (sizeof(double) + sizeof(int32_t));
        if (own_out) b += L * sizeof(double);
    }
    if (host_entry) {
        if (host_lam) b += L * sizeof(double);
        if (transform && host_out) b += L * sizeof(double);
        if (transform && host_arg) b += (size_t)du_out_rows(g) * sizeof(int32_t);
    }
    return b;
}
