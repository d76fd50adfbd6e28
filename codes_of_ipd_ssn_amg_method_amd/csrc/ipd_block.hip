// Several right-hand sides through one hierarchy: the solve phase of Class_AMG (Class_AMG.m:86-109)
// for every column of B at once, each column as if it were solved alone.
//
// The cycle is the launch-path amg_cycle (ipd_cycle.hip) with every vector widened to a block of
// W columns, W in {1, 2, 4, 8}: N x W row-major ("row-interleaved"), so the column index of one
// matrix entry fetches W contiguous doubles, and each matrix entry is read once per row walk for all
// W columns.  A launch of these kernels is bound by its dependent round trips, not its bytes
// (ipd_cycle_phases.h, "Latency structure"), so W columns should cost well under W launches.
//
// Kernels (each the block form of a single-vector one; template <W, STAGED>):
//   k_blk_smooth  Jacobi sweep or one bigraph Gauss-Seidel half (k_smooth); isnsp: one kernel-space
//                 scalar c per column, evaluated by every workgroup (1'r - (A1)'e) / xx
//   k_blk_resid   rr = r - A e (k_resid)          k_blk_rrc  r_c = P'r - T1 e (k_rrc)
//   k_blk_xfer    y = P'x, y += P x (k_xfer)      k_blk_top  x_new = x + e, r = b - A x_new (k_top)
//   k_blk_conv    per-column norms, Class_AMG's loop test and the active mask (conv_block)
//   k_blk_pcg     the coarsest Jacobi-PCG, one workgroup per column (k_pcg)
//   k_blk_in / k_blk_out   column-major <-> row-interleaved at entry and exit
// A gathered block of N*W <= STAGE_MAX doubles is staged in LDS; larger ones are gathered from L2.
// Matrices are the CSR arrays every level keeps; the padded copies, the fused single-workgroup
// program, the sub-cycle, the resident kernels, a mask operator and polynomial forms are not used.
//
// Frozen columns: a column whose loop has stopped is inactive.  k_blk_top leaves its x as it is and
// sets its residual to zero (so the following cycle gives it e = 0), k_blk_conv leaves its history
// and count alone.  Padding columns are zero and inactive from the start (res0 = 0).
// Reductions run in a fixed order inside one workgroup: no float atomics, the same bits run to run,
// and a column's bits do not depend on the other columns of its block.  One host read per cycle:
// the per-column history block.
#include "ipd_block.h"

// column-major (leading dimension ld, ncol columns) -> N x W interleaved, missing columns zero
__global__ __launch_bounds__(256) void k_blk_in(int N, int W, int ncol, const double* __restrict__ src,
                                                long long ld, double* __restrict__ dst) {
    const long long nw = (long long)N * W;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < nw; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / W), c = (int)(i - (long long)row * W);
        dst[i] = (src && c < ncol) ? src[c * ld + row] : 0.0;
    }
}

// N x W interleaved -> the first ncol columns of a column-major block
__global__ __launch_bounds__(256) void k_blk_out(int N, int W, int ncol, const double* __restrict__ src,
                                                 double* __restrict__ dst, long long ld) {
    const long long nw = (long long)N * ncol;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < nw; i += (long long)gridDim.x * 256) {
        const int c = (int)(i / N), row = (int)(i - (long long)c * N);
        dst[c * ld + row] = src[(size_t)row * W + c];
    }
}

template <int W>
static void solve_chunk(ipd_amg* h, const double* B, long long ldb, int ncol, const double* guess, double* X,
                        int32_t* it, double* rel_res, double* rel_resk, double* rhok) {
    BlockRun<W> run{h, h->ctx, block_state(h, W)};
    run.solve(B, ldb, ncol, guess, X, it, rel_res, rel_resk, rhok);
}

// all columns, in chunks of at most BLK_WMAX (device B, guess, X; host outputs)
static void amg_solve_multi_dev(ipd_amg* h, const double* B, long long ldb, long long nrhs, const double* guess,
                                double* X, int32_t* it, double* rel_res, double* rel_resk, double* rhok) {
    const long long hs = (long long)h->opts.maxit + 1;
    std::vector<double> rr((size_t)nrhs);
    for (long long j0 = 0; j0 < nrhs; j0 += BLK_WMAX) {
        const int ncol = (int)std::min<long long>(BLK_WMAX, nrhs - j0);
        const double* Bj = B + j0 * ldb;
        const double* gj = guess ? guess + j0 * ldb : nullptr;
        double* Xj = X + j0 * ldb;
        double* rk = rel_resk ? rel_resk + j0 * hs : nullptr;
        double* rh = rhok ? rhok + j0 * hs : nullptr;
        switch (block_width(ncol)) {
            case 1: solve_chunk<1>(h, Bj, ldb, ncol, gj, Xj, it + j0, rr.data() + j0, rk, rh); break;
            case 2: solve_chunk<2>(h, Bj, ldb, ncol, gj, Xj, it + j0, rr.data() + j0, rk, rh); break;
            case 4: solve_chunk<4>(h, Bj, ldb, ncol, gj, Xj, it + j0, rr.data() + j0, rk, rh); break;
            default: solve_chunk<8>(h, Bj, ldb, ncol, gj, Xj, it + j0, rr.data() + j0, rk, rh); break;
        }
    }
    if (rel_res) std::copy(rr.begin(), rr.end(), rel_res);
}

static void check_multi_args(ipd_amg* h, const double* B, long long ldb, long long nrhs, const double* X,
                             const int32_t* it) {
    IPD_REQUIRE(h && B && X && it, IPD_E_ARG, "NULL argument");
    IPD_REQUIRE(nrhs >= 1, IPD_E_ARG, "solve_multi: nrhs must be at least 1");
    IPD_REQUIRE(ldb >= (long long)h->L[1].A.nr, IPD_E_ARG, "solve_multi: ldb must be at least N");
    IPD_REQUIRE(amg_block_levels(h, nullptr), IPD_E_ARG, "solve_multi: the hierarchy is sharded over ranks");
}

extern "C" int ipd_amg_solve_multi_dev(ipd_amg* h, const double* B, int64_t ldb, int64_t nrhs,
                                       const double* guess, double* X, int32_t* it, double* rel_res,
                                       double* rel_resk, double* rhok) {
    return ipd_guard([&] {
        check_multi_args(h, B, ldb, nrhs, X, it);
        CallScope scope(h->ctx);
        amg_solve_multi_dev(h, B, ldb, nrhs, guess, X, it, rel_res, rel_resk, rhok);
    });
}

extern "C" int ipd_amg_solve_multi(ipd_amg* h, const double* B, int64_t ldb, int64_t nrhs, const double* guess,
                                   double* X, int32_t* it, double* rel_res, double* rel_resk, double* rhok) {
    return ipd_guard([&] {
        check_multi_args(h, B, ldb, nrhs, X, it);
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        const size_t n = (size_t)ldb * (size_t)nrhs;
        double* dB = ctx->scratch->alloc<double>(n);
        double* dX = ctx->scratch->alloc<double>(n);
        double* dg = nullptr;
        ctx->upload(dB, B, n);
        if (guess) {
            dg = ctx->scratch->alloc<double>(n);
            ctx->upload(dg, guess, n);
        }
        // rows N..ldb-1 of X are the caller's: carry them through
        if ((long long)ldb > (long long)h->L[1].A.nr) ctx->upload(dX, X, n);
        amg_solve_multi_dev(h, dB, ldb, nrhs, dg, dX, it, rel_res, rel_resk, rhok);
        ctx->fetch(dX, X, n);
    });
}
