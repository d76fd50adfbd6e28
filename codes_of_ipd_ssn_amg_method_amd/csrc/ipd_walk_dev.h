// The frame of the kernels that walk an m x n array by column groups (ipd_walk_geo.h): k_pa_rows
// and k_pa_cols (ipd_plan_apply.hip), k_du_rows, k_du_cols and k_du_eval (ipd_dual.hip), k_du_both and k_du_eval2
// (ipd_bracket.hip) and, with the driver's own geometry, k_plan_count and k_plan_fill (ipd_plan.hip); k_rd_last
// (ipd_round.hip) takes the workgroup sums.  Device
// only, everything inlined and decided at compile time.  The helpers are as small as they are on purpose: these
// kernels are held to the machine code they were measured with, and that code moves with the shape of the source --
// a helper that owns the loop over a chunk's 16 loads changes the address arithmetic, so walk_place gives the place
// and the kernels keep the unrolled loop; a slot computed before its use changes the schedule, so it is a function;
// and k_rd_walk (ipd_round.hip) writes the frame out, because two of its passes change with any of it.
//
// Lanes run along i (coalesced): thread tid of row block ib has row ib*TR + tid, a wave 64 consecutive rows.  Per
// chunk of TC columns a lane has 16 loads per array in flight, of clamped places so that they need no branch; a
// padding lane (row >= m) and a clamped column (>= n) read the last row resp. column and their values are masked by
// the caller.  No LDS tile, no barrier inside the chunk loop.  What is uniform over the wave per column (q, a
// multiplier, the coordinates) is fetched by lane l for column walk_lane_col and handed round with __shfl: 16 uniform
// loads per array would hold scalar registers the kernels cannot spare.  The 16 column results of a chunk over the
// wave's 64 rows come out of colsum16's butterfly (ipd_apd_tiles.h) or colmax16's (ipd_dual_dev.h), which leaves the
// result of column j0 + colsum_index(l) in lane l < 16.
#pragma once

#include "ipd_apd_tiles.h"
#include "ipd_walk_geo.h"

struct WalkLane {
    int tid, wv, lane;   // thread of the workgroup, its wave, its lane
    int ib, grp;         // row block and column group of the workgroup
    int i;               // the thread's row
    bool in_i;           // i < m
    int ic;              // the row its loads read: i, the last row for a padding lane
    // the segment slot of the thread's wave: of a segment without rows too, its partials are the neutral element
    __device__ __forceinline__ int slot() const { return walk_slot(ib, wv); }
};

__device__ __forceinline__ WalkLane walk_lane(int m) {
    WalkLane t;
    t.tid = threadIdx.x;
    t.wv = t.tid >> 6;
    t.lane = t.tid & 63;
    t.ib = blockIdx.x;
    t.grp = blockIdx.y;
    t.i = t.ib * TR + t.tid;
    t.in_i = t.i < m;
    t.ic = t.in_i ? t.i : m - 1;
    return t;
}

// where the loads of column j0 + jj of a chunk read row t.ic of an m x n array: the column clamped at n - 1, so that
// the 16 loads per array of a chunk need no branch and go out together
template <class G>
__device__ __forceinline__ size_t walk_place(const WalkLane& t, const G& g, int j0, int jj) {
    const int j = min(j0 + jj, g.n - 1);
    return (size_t)j * g.m + t.ic;
}

// the column whose per-column values this lane fetches, clamped; __shfl(value, jj) is that of column j0 + jj
template <class G>
__device__ __forceinline__ int walk_lane_col(const WalkLane& t, const G& g, int j0) {
    return min(j0 + (t.lane & (TC - 1)), g.n - 1);
}

// does this lane hold a butterfly's result of a column below n?  col: that column
template <class G>
__device__ __forceinline__ bool walk_col_owner(const WalkLane& t, const G& g, int j0, int& col) {
    col = j0 + colsum_index(t.lane);
    return t.lane < 16 && col < g.n;
}

// N sums over the workgroup in a fixed shape: wave_sum's tree, lane 0 of every wave to red[APD_WAVES * N], a barrier;
// after it walk_waves_total adds the four waves' sums of number k in order
template <int N>
__device__ __forceinline__ void walk_wave_sums(int lane, int wv, const double (&s)[N], double* red) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double w = wave_sum(s[k]);
        if (lane == 0) red[wv * N + k] = w;
    }
    __syncthreads();
}
template <int N>
__device__ __forceinline__ double walk_waves_total(const double* red, int k) {
    double r = red[k];
#pragma unroll
    for (int w = 1; w < APD_WAVES; ++w) r += red[w * N + k];
    return r;
}

// is x an entry of the plan at the threshold tol?  A NaN fails the comparison and is kept, as MATLAB's sparse() keeps it
__device__ __forceinline__ bool walk_keep(double x, double tol) { return !(fabs(x) <= tol); }
// max(v, 0); a NaN becomes 0
__device__ __forceinline__ double walk_pos(double v) { return v > 0.0 ? v : 0.0; }
