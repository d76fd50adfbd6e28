// Device side of the drivers' mn-sized passes, shared by their units (ipd_apd_passes.hip, ipd_apd_warm.hip) and by
// ipd_plan.hip, which writes the same partial sums: the tile walker k_tiles<Op>, its column butterfly, and what the
// epilogues read the partials with.  Device only; the geometry is ipd_apd_geo.h's.
//
// Layout: x(i,j) = x[i + j*m] (MATLAB's reshape(x,m,n)); a wave owns 64 rows x (16*reps)
// columns, lanes run along i (coalesced), 16 independent loads in flight per lane and array.
// Row sums accumulate in registers, the 16 column sums of a chunk come out of a register
// butterfly (k_tiles); partial sums are combined by small epilogue kernels in a fixed order
// (deterministic, no float atomics), which also do all O(m+n) vector work.
#pragma once

#include "ipd_apd_geo.h"
#include "ipd_cost_plan.h"
#include "ipd_cycle_dev.h"

// TR, TC, Geo and make_geo: ipd_apd_geo.h
constexpr int NSC = 8;         // scalar accumulators per workgroup

// problem constants shared by all passes
struct Prob {
    int cls2;            // 0: class 1 (box prox), 1: class 2 (max(0,.), phi row, tails)
    int m, n;
    const double* p;
    const double* q;
    const double* c;
    const double* phi;   // class 2
    const double* gama;  // class 1, NULL -> gs
    double gs;
};

__device__ __forceinline__ double prox_of(const Prob& P, double x, double g) {
    // prox = @(x) min(max(0,x),gama) (Class1 :32) / max(0,x) (Class2 :29)
    const double t = x > 0.0 ? x : 0.0;
    return P.cls2 ? t : (t < g ? t : g);
}

// ---------------------------------------------------------------------------
// where an op that reads c(i,j) takes it from: a compile-time choice of the op
// ---------------------------------------------------------------------------
// the stored matrix (P.c, or PlanCount::c): nothing per row or column, the value is what the op loaded
struct CostStored {
    static constexpr bool FREE = false;
    struct Row {};
    struct Col {};
    __device__ __forceinline__ void row(Row&, int) const {}
    __device__ __forceinline__ void col(Col&, int) const {}
    __device__ __forceinline__ void col_of_lane(Col&, const Col&, int) const {}
    __device__ __forceinline__ double value(double stored, const Row&, const Col&) const { return stored; }
};
// none stored: the row's D coordinates are registers of the lane, the column's are wave-uniform, and the entry
// is folded by cost_src_value, the code k_cost_build stores an entry with.  The coordinates are never written
// while a workspace lives, so the column loads go through the constant address space: a uniform address there
// is a scalar load even in a kernel that stores elsewhere.
template <int D>
struct CostFree {
    static constexpr bool FREE = true;
    CostSrc s;
    struct Row {
        double x[D];
    };
    struct Col {
        double y[D];
    };
    __device__ __forceinline__ void row(Row& r, int i) const { cost_src_row<D>(s, i, r.x); }
    __device__ __forceinline__ void col(Col& c, int j) const {
        typedef const double __attribute__((address_space(4))) * ConstPtr;
        ConstPtr const ys = (ConstPtr)s.ys;
#pragma unroll
        for (int k = 0; k < D; ++k) c.y[k] = ys[(size_t)k * s.n + j];
    }
    // the coordinates lane `src_lane` fetched with col(), in every lane
    __device__ __forceinline__ void col_of_lane(Col& c, const Col& mine, int src_lane) const {
#pragma unroll
        for (int k = 0; k < D; ++k) c.y[k] = __shfl(mine.y[k], src_lane);
    }
    __device__ __forceinline__ double value(double, const Row& r, const Col& c) const {
        return cost_src_value<D>(s, r.x, c.y);
    }
};

// multiplier, optionally a line-search trial point lam + step*zeta (:189,200)
struct Lam {
    const double* base;
    const double* zeta;  // NULL -> base
    double step;
    __device__ __forceinline__ double at(int t) const {
        return zeta ? base[t] + step * zeta[t] : base[t];
    }
};

// ---------------------------------------------------------------------------
// tile walker
// ---------------------------------------------------------------------------
// 16 values per lane (one per column of a chunk) -> the 16 column sums over the wave's 64 rows.
// A butterfly reduce-scatter over lane bits 0..3 halves the live values at every step (8+4+2+1
// exchanges) and two more exchanges add the four 16-lane rows: 17 exchanges instead of 16 full
// wave reductions (tools/ubench_eval.hip: 5.8 -> 6.1 TB/s at m=n=4096, 2.2 -> 2.6 at 1024).
// On return lane l < 16 holds the sum of column colsum_index(l).
__device__ __forceinline__ double colsum16(const double (&xv)[TC], int lane) {
    double a8[8], a4[4], a2[2], a1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const bool hi = lane & 1;
        a8[k] = (hi ? xv[k + 8] : xv[k]) + __shfl_xor(hi ? xv[k] : xv[k + 8], 1);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool hi = lane & 2;
        a4[k] = (hi ? a8[k + 4] : a8[k]) + __shfl_xor(hi ? a8[k] : a8[k + 4], 2);
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const bool hi = lane & 4;
        a2[k] = (hi ? a4[k + 2] : a4[k]) + __shfl_xor(hi ? a4[k] : a4[k + 2], 4);
    }
    {
        const bool hi = lane & 8;
        a1 = (hi ? a2[1] : a2[0]) + __shfl_xor(hi ? a2[0] : a2[1], 8);
    }
    a1 += __shfl_xor(a1, 16);
    a1 += __shfl_xor(a1, 32);
    return a1;
}
__device__ __forceinline__ int colsum_index(int lane) {
    return ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3);
}

namespace {   // every unit instantiates the walker for its own ops

template <class Op>
__global__ __launch_bounds__(256) void k_tiles(const Op op, const Geo g,
                                               double* __restrict__ lpart,
                                               double* __restrict__ rpart,
                                               double* __restrict__ spart) {
    // Every wave owns 64 consecutive rows and walks its columns alone: row sums stay in a
    // register, the column sums over the wave's rows come out of a register butterfly -- no
    // LDS tile, no barrier inside the loop (the first version transposed 256x16 tiles through
    // LDS and stalled three times per tile: 2.0 TB/s at m=n=4096).
    __shared__ double red[4 * NSC];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ib = blockIdx.x, jg = blockIdx.y;
    const int i = ib * TR + tid;
    const bool in_i = i < g.m;
    const int ic = in_i ? i : g.m - 1;
    const double pi = in_i ? op.P.p[i] : 0.0;
    typename Op::RowC rc;
    op.row_const(rc, ic);
    double sc[NSC];
#pragma unroll
    for (int k = 0; k < NSC; ++k) sc[k] = 0.0;
    double lacc = 0.0;
    double* const rrow = rpart + ((size_t)ib * 4 + wv) * g.n;
    for (int rep = 0; rep < g.reps; ++rep) {
        const int j0 = (jg * g.reps + rep) * TC;
        if (j0 >= g.n) break;  // uniform
        double xv[TC];
        // loads are issued Op::FC columns at a time: enough bytes in flight per lane without
        // spilling the ops that stream six or seven arrays
#pragma unroll
        for (int c0 = 0; c0 < TC; c0 += Op::FC) {
            typename Op::Raw raw[Op::FC];
            typename Op::ColC cc[Op::FC];
#pragma unroll
            for (int jj = 0; jj < Op::FC; ++jj) {
                const int j = min(j0 + c0 + jj, g.n - 1);
                op.fetch(raw[jj], (size_t)j * g.m + ic);
                // per-column uniforms (scalar loads) up front, with a clamped index: inside the
                // bounds check below they could not be hoisted and serialised every column
                op.col_const(cc[jj], j);
            }
#pragma unroll
            for (int jj = 0; jj < Op::FC; ++jj) {
                const int j = j0 + c0 + jj;
                double x = 0.0;
                if (in_i && j < g.n) {
                    x = op.compute(raw[jj], rc, cc[jj], (size_t)j * g.m + i, sc);
                    lacc += x * cc[jj].q;
                }
                xv[c0 + jj] = x * pi;
            }
        }
        if (Op::NEED_AX) {
            const double cs = colsum16(xv, lane);
            const int col = j0 + colsum_index(lane);
            if (lane < 16 && col < g.n) rrow[col] = cs;
        }
    }
    if (Op::NEED_AX && in_i) lpart[(size_t)jg * g.m + i] = lacc;
#pragma unroll
    for (int k = 0; k < NSC; ++k) {
        const double w = wave_sum(sc[k]);
        if (lane == 0) red[wv * NSC + k] = w;
    }
    __syncthreads();
    if (tid < NSC) {
        const int blk = jg * gridDim.x + ib;
        spart[(size_t)blk * NSC + tid] =
            red[tid] + red[NSC + tid] + red[2 * NSC + tid] + red[3 * NSC + tid];
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// what the epilogues (one workgroup of 1024 threads) read the partials with
// ---------------------------------------------------------------------------
struct Parts {
    Geo g;
    const double* lpart;
    const double* rpart;
    const double* spart;
    int nblk;
};

// sum of the partials of one entry of A*x, in a fixed order; loads go out 32 at a time (a
// plain loop pays one L2/HBM round trip per partial: 64 of them made this epilogue 47 us)
__device__ __forceinline__ double sum_strided(const double* __restrict__ base, int count,
                                              size_t stride) {
    double s = 0.0;
    int k = 0;
    for (; k + 32 <= count; k += 32) {
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = base[(size_t)(k + u) * stride];
#pragma unroll
        for (int u = 0; u < 32; ++u) s += v[u];
    }
    for (; k + 8 <= count; k += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(k + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < count; ++k) s += base[(size_t)k * stride];
    return s;
}

__device__ __forceinline__ double ax_entry(const Parts& pt, int t) {
    if (t < pt.g.n) return sum_strided(pt.rpart + t, 4 * pt.g.nib, (size_t)pt.g.n);
    return sum_strided(pt.lpart + (t - pt.g.n), pt.g.njg, (size_t)pt.g.m);
}

__device__ __forceinline__ double scal_total(const Parts& pt, int slot, double* red) {
    double a = 0.0;
    for (int b = threadIdx.x; b < pt.nblk; b += BT) a += pt.spart[(size_t)b * NSC + slot];
    return block_sum(a, red);
}
