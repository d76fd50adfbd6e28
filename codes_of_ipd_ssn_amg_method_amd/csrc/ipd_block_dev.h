// Device helpers of the block form of the launch-path cycle, shared by the block kernels (ipd_block.hip) and the
// block PCG's (ipd_block_krylov.hip): N x W row-interleaved blocks, W contiguous doubles per row, and the CSR row
// walk against such a block.  Device only; no kernel.
#pragma once

#include "ipd_cycle_dev.h"
#include "ipd_cycle_phases.h"
#include "ipd_limits.h"   // BLK_WMAX

static constexpr int BLK_WAVES = BT / 64;

// W contiguous doubles (16-byte aligned for W >= 2)
template <int W>
__device__ __forceinline__ void blk_load(const double* p, double (&y)[W]) {
    if constexpr (W == 1) {
        y[0] = p[0];
    } else {
#pragma unroll
        for (int c = 0; c < W; c += 2) {
            const double2 v = *reinterpret_cast<const double2*>(p + c);
            y[c] = v.x;
            y[c + 1] = v.y;
        }
    }
}
template <int W>
__device__ __forceinline__ void blk_store(double* p, const double (&y)[W]) {
    if constexpr (W == 1) {
        p[0] = y[0];
    } else {
#pragma unroll
        for (int c = 0; c < W; c += 2) *reinterpret_cast<double2*>(p + c) = make_double2(y[c], y[c + 1]);
    }
}

// s[c] += sum_u a_u x(j_u)[c] over one batch of a row
template <int W, class GAT>
__device__ __forceinline__ void blk_batch(const RowBatch& bt, GAT gat, double (&s)[W]) {
#pragma unroll
    for (int u = 0; u < ROW_U; ++u) {
        double y[W];
        gat(bt.j[u], y);
#pragma unroll
        for (int c = 0; c < W; ++c) s[c] += bt.a[u] * y[c];
    }
}

// this lane's share of row `row` of a CSR matrix against the block (invalid rows: zeros)
template <int W, class GAT>
__device__ __forceinline__ void blk_row(const int* __restrict__ rp, const int* __restrict__ ci,
                                        const double* __restrict__ va, int row, bool valid, int gl, int L,
                                        GAT gat, double (&s)[W]) {
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] = 0.0;
    const int rowc = valid ? row : 0;
    const int e0 = rp[rowc], e1 = valid ? rp[rowc + 1] : e0;
    for (int t = e0 + gl; t < e1; t += ROW_U * L) {
        RowBatch bt;
        batch_load_csr(bt, ci, va, t, e1, L);
        blk_batch<W>(bt, gat, s);
    }
}

// sums over aligned groups of L lanes (result in every lane of the group); red: W x BLK_WAVES
template <int W>
__device__ __forceinline__ void blk_reduce_rows(double (&s)[W], int L, double* red) {
    if (L <= 64) {
#pragma unroll
        for (int c = 0; c < W; ++c) s[c] = subwave_sum(s[c], L);
        return;
    }
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < W; ++c) s[c] = wave_sum(s[c]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) red[c * BLK_WAVES + w] = s[c];
    }
    __syncthreads();
    const int wpg = L >> 6, g0 = (threadIdx.x / L) * wpg;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double t = 0.0;
        for (int k = 0; k < wpg; ++k) t += red[c * BLK_WAVES + g0 + k];
        s[c] = t;
    }
    __syncthreads();
}

// Row walk of rows [row0, row1) of a CSR matrix against the block that load(j, y) gives for column
// index j (ncols of them; copied into LDS first when STAGED), then epi(row, s) in the row's first lane.
// walk == false: s = 0 without touching the matrix.
template <int W, bool STAGED, class LOAD, class EPI>
__device__ __forceinline__ void blk_walk(const int* rp, const int* ci, const double* va, int L, int ncols,
                                         int row0, int row1, bool walk, LOAD load, EPI epi, double* red,
                                         double* xs) {
    const int tid = threadIdx.x, b = blockIdx.x, G = gridDim.x;
    const int gpb = BT / L, g = tid / L, gl = tid - g * L;
    const bool uni = L >= 64;
    if (STAGED && walk) {
        for (int j = tid; j < ncols; j += BT) {
            double y[W];
            load(j, y);
            blk_store<W>(xs + (size_t)j * W, y);
        }
        __syncthreads();
    }
    auto glds = [&](int j, double (&y)[W]) { blk_load<W>(xs + (size_t)j * W, y); };
    const int niter = (row1 - row0 + G * gpb - 1) / (G * gpb);
    for (int it = 0; it < niter; ++it) {
        const int row = uniform_if(row0 + (it * G + b) * gpb + g, uni);
        const bool valid = row < row1;
        double s[W];
        if (walk) {
            if (STAGED)
                blk_row<W>(rp, ci, va, row, valid, gl, L, glds, s);
            else
                blk_row<W>(rp, ci, va, row, valid, gl, L, load, s);
        } else {
#pragma unroll
            for (int c = 0; c < W; ++c) s[c] = 0.0;
        }
        blk_reduce_rows<W>(s, L, red);
        if (valid && gl == 0) epi(row, s);
    }
}
