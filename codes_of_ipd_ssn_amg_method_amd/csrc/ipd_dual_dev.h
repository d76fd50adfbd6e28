// Device helpers of the dual certificate that two units' kernels share (ipd_dual.hip, ipd_bracket.hip; DESIGN.md
// sections 4k and 4m): the two keys a transform and an evaluation reduce under, and colmax16's butterfly.  Device only,
// everything inlined; the units that include this keep the kernels they define (ipd_apd_state.h).
#pragma once

#include "ipd_dual_geo.h"
#include "ipd_walk_dev.h"

namespace {

// TR, TC: ipd_apd_geo.h; colsum_index: ipd_apd_tiles.h
constexpr int DU_NOIDX = 0x7fffffff;                  // the index of a padding lane: behind every row
constexpr long long DU_NOPLACE = 0x7fffffffffffffffLL;   // the place of "no entry"

// (value descending, index ascending): does (bv, bi) come before (av, ai)?
__device__ __forceinline__ bool du_before(double bv, int bi, double av, int ai) {
    return bv > av || (bv == av && bi < ai);
}
__device__ __forceinline__ void du_merge(double& v, int& i, double ov, int oi) {
    const bool take = du_before(ov, oi, v, i);
    v = take ? ov : v;
    i = take ? oi : i;
}
// (value ascending, place ascending)
__device__ __forceinline__ void du_merge_min(double& v, long long& i, double ov, long long oi) {
    const bool take = ov < v || (ov == v && oi < i);
    v = take ? ov : v;
    i = take ? oi : i;
}

// 16 candidates per lane (one per column of a chunk, all of row `row`) -> the 16 column maxima over the wave's 64
// rows with the rows that reach them: colsum16's butterfly (ipd_apd_tiles.h) on the key.  On return lane l < 16
// holds the maximum of column colsum_index(l).
__device__ __forceinline__ void colmax16(const double (&xv)[TC], int row, int lane, double& out_v, int& out_i) {
    double v8[8], v4[4], v2[2], v1;
    int i8[8], i4[4], i2[2], i1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool hi = lane & 1;
        v8[k] = hi ? xv[k + 8] : xv[k];
        i8[k] = row;
        du_merge(v8[k], i8[k], __shfl_xor(hi ? xv[k] : xv[k + 8], 1), __shfl_xor(row, 1));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool hi = lane & 2;
        v4[k] = hi ? v8[k + 4] : v8[k];
        i4[k] = hi ? i8[k + 4] : i8[k];
        du_merge(v4[k], i4[k], __shfl_xor(hi ? v8[k] : v8[k + 4], 2), __shfl_xor(hi ? i8[k] : i8[k + 4], 2));
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool hi = lane & 4;
        v2[k] = hi ? v4[k + 2] : v4[k];
        i2[k] = hi ? i4[k + 2] : i4[k];
        du_merge(v2[k], i2[k], __shfl_xor(hi ? v4[k] : v4[k + 2], 4), __shfl_xor(hi ? i4[k] : i4[k + 2], 4));
    }
    {
        const bool hi = lane & 8;
        v1 = hi ? v2[1] : v2[0];
        i1 = hi ? i2[1] : i2[0];
        du_merge(v1, i1, __shfl_xor(hi ? v2[0] : v2[1], 8), __shfl_xor(hi ? i2[0] : i2[1], 8));
    }
    du_merge(v1, i1, __shfl_xor(v1, 16), __shfl_xor(i1, 16));
    du_merge(v1, i1, __shfl_xor(v1, 32), __shfl_xor(i1, 32));
    out_v = v1;
    out_i = i1;
}

}  // namespace
