// Several right-hand sides through one hierarchy: the solve phase of Class_AMG (Class_AMG.m:86-109)
// for every column of B at once, each column as if it were solved alone.
//
// The cycle is the launch-path amg_cycle (ipd_cycle.hip) with every vector widened to a block of
// W columns, W in {1, 2, 4, 8}: N x W row-major ("row-interleaved"), so the column index of one
// matrix entry fetches W contiguous doubles, and each matrix entry is read once per row walk for all
// W columns.  A launch of these kernels is bound by its dependent round trips, not its bytes
// (ipd_cycle_phases.h, "Latency structure"), so W columns should cost well under W launches.
//
// This is the only unit that instantiates and launches k_blk_*; ipd_block_krylov.hip runs the block cycle through
// the host functions of ipd_block_state.h.  The device helpers both share are in ipd_block_dev.h.
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
#include "ipd_block_state.h"

#include <cmath>

#include "ipd_block_dev.h"

static constexpr int HB = 8;   // doubles of a column's history record (see k_blk_conv)
enum { HB_RES0, HB_RES, HB_PREV, HB_REL, HB_RHO, HB_ACT, HB_CNT };

// sums over the whole workgroup, result in every thread
template <int W>
__device__ __forceinline__ void blk_block_sum(double (&v)[W], double* red) {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = wave_sum(v[c]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) red[c * BLK_WAVES + w] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < BLK_WAVES; ++k) t += red[c * BLK_WAVES + k];
        v[c] = t;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// smoother sweep: Jacobi, or one half of the bigraph Gauss-Seidel sweep        MG_Vcycle.m:14-25
// ---------------------------------------------------------------------------
struct BlkSmoothArgs {
    const int* rp;
    const int* ci;
    const double* va;
    int N, L;
    int row0, row1;   // rows updated
    int u0, u1;       // columns in [u0,u1) read `win` (first-half result), others `eold`
    const double* r;
    const double* dinv;
    const double* Axi;
    const double* xx;
    const double* eold;
    const double* win;
    double* enew;
    double* wout;     // NULL: not written
    int isnsp;
    int eold_zero;    // eold is identically zero and is not read
};

template <int W, bool STAGED>
__global__ __launch_bounds__(BT) void k_blk_smooth(BlkSmoothArgs a) {
    __shared__ double red[W * BLK_WAVES];
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const bool ez = a.eold_zero != 0;
    const int u0 = a.u0, u1 = a.u1;
    const bool skip = ez && u0 >= u1;   // nothing to gather: A e == 0
    const bool nsp = a.isnsp != 0;
    const double* __restrict__ eold = a.eold;
    const double* __restrict__ win = a.win;
    auto load = [&](int j, double (&y)[W]) {
        const bool inw = j >= u0 && j < u1;
        if (u1 > u0) {   // uniform
            blk_load<W>((inw ? win : eold) + (size_t)j * W, y);
        } else {
            blk_load<W>(eold + (size_t)j * W, y);
        }
        if (ez && !inw) {
#pragma unroll
            for (int c = 0; c < W; ++c) y[c] = 0.0;
        }
    };
    // c = (1'r - (A1)'e_old) / xx per column, kept in LDS (W uniform values would take SGPRs)
    __shared__ __attribute__((aligned(16))) double csh[W];   // MG_Vcycle.m:18-19 (read as double2)
    if (nsp) {
        double cv[W];
#pragma unroll
        for (int c = 0; c < W; ++c) cv[c] = 0.0;
        for (int j = threadIdx.x; j < a.N; j += BT) {
            double rv[W], ev[W];
            blk_load<W>(a.r + (size_t)j * W, rv);
            if (ez) {
#pragma unroll
                for (int c = 0; c < W; ++c) ev[c] = 0.0;
            } else {
                blk_load<W>(eold + (size_t)j * W, ev);
            }
            const double ax = a.Axi[j];
#pragma unroll
            for (int c = 0; c < W; ++c) cv[c] += rv[c] - ax * ev[c];
        }
        blk_block_sum<W>(cv, red);
        if (threadIdx.x == 0) {
            const double xxv = a.xx[0];
#pragma unroll
            for (int c = 0; c < W; ++c) csh[c] = cv[c] / xxv;
        }
    } else if (threadIdx.x < W) {
        csh[threadIdx.x] = 0.0;
    }
    __syncthreads();
    auto epi = [&](int row, const double (&s)[W]) {
        double rv[W], eo[W];
        blk_load<W>(a.r + (size_t)row * W, rv);
        if (ez) {
#pragma unroll
            for (int c = 0; c < W; ++c) eo[c] = 0.0;
        } else {
            blk_load<W>(eold + (size_t)row * W, eo);   // row is never inside [u0,u1)
        }
        const double dv = a.dinv[row];
        const double axi = nsp ? a.Axi[row] : 0.0;
        double cv[W], wv[W], en[W];
        blk_load<W>(csh, cv);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const double g_i = rv[c] - s[c] - axi * cv[c];
            wv[c] = eo[c] + dv * g_i;   // e + R*(g - Axi*c)
            en[c] = wv[c] + cv[c];      //   ... + xi*c
        }
        if (a.wout) blk_store<W>(a.wout + (size_t)row * W, wv);
        blk_store<W>(a.enew + (size_t)row * W, en);
    };
    blk_walk<W, STAGED>(a.rp, a.ci, a.va, a.L, a.N, a.row0, a.row1, !skip, load, epi, red, xs);
}

// ---------------------------------------------------------------------------
// rr = r - A e                                                                  MG_Vcycle.m:27
// ---------------------------------------------------------------------------
struct BlkWalkArgs {
    const int* rp;
    const int* ci;
    const double* va;
    int L, nrows, ncols;
    const double* x;    // gathered block
    const double* x2;   // resid: r ; top: e (NULL: x_new = x) ; rrc: e
    const double* b;    // top: right-hand side
    double* y;          // resid: rr ; xfer: y ; top: r ; rrc: coarse right-hand side
    double* y2;         // top: x_new
    const double* hist; // top: per-column records (HB_ACT); NULL: every column active
    int add;            // xfer: 1 = prolongation (y += M x)
    // rrc: T1 = P'A (CSR, same rows)
    const int* rp2;
    const int* ci2;
    const double* va2;
};

template <int W, bool STAGED>
__global__ __launch_bounds__(BT) void k_blk_resid(BlkWalkArgs a) {
    __shared__ double red[W * BLK_WAVES];
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const double* __restrict__ e = a.x;
    auto load = [&](int j, double (&y)[W]) { blk_load<W>(e + (size_t)j * W, y); };
    auto epi = [&](int row, const double (&s)[W]) {
        double rv[W];
        blk_load<W>(a.x2 + (size_t)row * W, rv);
#pragma unroll
        for (int c = 0; c < W; ++c) rv[c] = rv[c] - s[c];
        blk_store<W>(a.y + (size_t)row * W, rv);
    };
    blk_walk<W, STAGED>(a.rp, a.ci, a.va, a.L, a.ncols, 0, a.nrows, true, load, epi, red, xs);
}

// y = M x (restriction, M = P') or y += M x (prolongation, M = P)               MG_Vcycle.m:27,31
template <int W, bool STAGED>
__global__ __launch_bounds__(BT) void k_blk_xfer(BlkWalkArgs a) {
    __shared__ double red[W * BLK_WAVES];
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const double* __restrict__ x = a.x;
    auto load = [&](int j, double (&y)[W]) { blk_load<W>(x + (size_t)j * W, y); };
    auto epi = [&](int row, const double (&s)[W]) {
        double yv[W];
        if (a.add) {
            blk_load<W>(a.y + (size_t)row * W, yv);
#pragma unroll
            for (int c = 0; c < W; ++c) yv[c] = yv[c] + s[c];
        } else {
#pragma unroll
            for (int c = 0; c < W; ++c) yv[c] = s[c];
        }
        blk_store<W>(a.y + (size_t)row * W, yv);
    };
    blk_walk<W, STAGED>(a.rp, a.ci, a.va, a.L, a.ncols, 0, a.nrows, true, load, epi, red, xs);
}

// r_c = P'r - (P'A) e: one walk over the rows of P' (against r) and of T1 (against e)   MG_Vcycle.m:27
template <int W, bool STAGED>
__global__ __launch_bounds__(BT) void k_blk_rrc(BlkWalkArgs a) {
    __shared__ double red[W * BLK_WAVES];
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const int tid = threadIdx.x, b = blockIdx.x, G = gridDim.x;
    const int L = a.L, gpb = BT / L, g = tid / L, gl = tid - g * L;
    const bool uni = L >= 64;
    const int ncols = a.ncols;
    const double* __restrict__ r = a.x;
    const double* __restrict__ e = a.x2;
    double* xe = xs + (size_t)ncols * W;
    if (STAGED) {
        for (int j = tid; j < ncols; j += BT) {
            double y[W], z[W];
            blk_load<W>(r + (size_t)j * W, y);
            blk_load<W>(e + (size_t)j * W, z);
            blk_store<W>(xs + (size_t)j * W, y);
            blk_store<W>(xe + (size_t)j * W, z);
        }
        __syncthreads();
    }
    auto rglobal = [&](int j, double (&y)[W]) { blk_load<W>(r + (size_t)j * W, y); };
    auto eglobal = [&](int j, double (&y)[W]) { blk_load<W>(e + (size_t)j * W, y); };
    auto rlds = [&](int j, double (&y)[W]) { blk_load<W>(xs + (size_t)j * W, y); };
    auto elds = [&](int j, double (&y)[W]) { blk_load<W>(xe + (size_t)j * W, y); };
    const int niter = (a.nrows + G * gpb - 1) / (G * gpb);
    for (int it = 0; it < niter; ++it) {
        const int row = uniform_if((it * G + b) * gpb + g, uni);
        const bool valid = row < a.nrows;
        double s1[W], s2[W];
        if (STAGED) {
            blk_row<W>(a.rp, a.ci, a.va, row, valid, gl, L, rlds, s1);
            blk_row<W>(a.rp2, a.ci2, a.va2, row, valid, gl, L, elds, s2);
        } else {
            blk_row<W>(a.rp, a.ci, a.va, row, valid, gl, L, rglobal, s1);
            blk_row<W>(a.rp2, a.ci2, a.va2, row, valid, gl, L, eglobal, s2);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) s1[c] = s1[c] - s2[c];
        blk_reduce_rows<W>(s1, L, red);
        if (valid && gl == 0) blk_store<W>(a.y + (size_t)row * W, s1);
    }
}

// top of the Class_AMG loop: x_new = x + e ; r = b - A x_new.  Inactive columns: x_new = x, r = 0.
template <int W, bool STAGED>
__global__ __launch_bounds__(BT) void k_blk_top(BlkWalkArgs a) {
    __shared__ double red[W * BLK_WAVES];
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const double* __restrict__ x = a.x;
    const double* __restrict__ e = a.x2;
    unsigned act = 0;   // bit c: column c active
#pragma unroll
    for (int c = 0; c < W; ++c) act |= (a.hist ? a.hist[c * HB + HB_ACT] != 0.0 : true) ? 1u << c : 0u;
    auto load = [&](int j, double (&y)[W]) {
        blk_load<W>(x + (size_t)j * W, y);
        if (e) {
            double ev[W];
            blk_load<W>(e + (size_t)j * W, ev);
#pragma unroll
            for (int c = 0; c < W; ++c) y[c] = (act >> c & 1u) ? y[c] + ev[c] : y[c];
        }
    };
    auto epi = [&](int row, const double (&s)[W]) {
        double xo[W], bv[W], rv[W];
        load(row, xo);
        blk_load<W>(a.b + (size_t)row * W, bv);
#pragma unroll
        for (int c = 0; c < W; ++c) rv[c] = (act >> c & 1u) ? bv[c] - s[c] : 0.0;
        blk_store<W>(a.y + (size_t)row * W, rv);
        blk_store<W>(a.y2 + (size_t)row * W, xo);
    };
    blk_walk<W, STAGED>(a.rp, a.ci, a.va, a.L, a.ncols, 0, a.nrows, true, load, epi, red, xs);
}

// ---------------------------------------------------------------------------
// per-column loop test (Class_AMG.m:89-106): one workgroup.  Record of column c, hist[c*HB ..]:
//   res0, res, previous res, rel_res, rhok, active, cycles done.
// Thread t only ever touches column t % W (W divides BT), so the partial sums reduce per column in a
// fixed tree order.
// ---------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(BT) void k_blk_conv(const double* __restrict__ r, int n, double* hist, int first,
                                                 double retol, double maxit) {
    __shared__ double red[BT];
    const int tid = threadIdx.x;
    const long long nw = (long long)n * W;
    double s = 0.0;
    for (long long i = tid; i < nw; i += BT) {
        const double v = r[i];
        s += v * v;
    }
    red[tid] = s;
    for (int half = BT / 2; half >= W; half >>= 1) {
        __syncthreads();
        if (tid < half) red[tid] = red[tid] + red[tid + half];
    }
    __syncthreads();
    if (tid < W) {
        double* H = hist + tid * HB;
        const double res = sqrt(red[tid]);
        if (first) {                                                             // :89
            H[HB_RES0] = res;
            H[HB_RES] = res;
            H[HB_PREV] = res;
            H[HB_REL] = 1.0;
            H[HB_RHO] = 0.0;
            H[HB_CNT] = 0.0;
            H[HB_ACT] = (res != 0.0 && 1.0 > retol && 1.0 <= maxit) ? 1.0 : 0.0;  // :91, :95
        } else if (H[HB_ACT] != 0.0) {
            const double prev = H[HB_RES];
            const double rel = res / H[HB_RES0];                                 // :103
            const double rho = res / prev;                                       // :105
            const double cnt = H[HB_CNT] + 1.0;
            H[HB_PREV] = prev;
            H[HB_RES] = res;
            H[HB_REL] = rel;
            H[HB_RHO] = rho;
            H[HB_CNT] = cnt;
            H[HB_ACT] = (!(rho > 1.0) && rel > retol && cnt + 1.0 <= maxit) ? 1.0 : 0.0;  // :95, :106
        }
    }
}

// ---------------------------------------------------------------------------
// coarsest level: PCG(A, r) with Jacobi (PCG.m:68-87), workgroup c solves column c from a zero guess
// ---------------------------------------------------------------------------
struct BlkPcgArgs {
    int N, L;
    const int* rp;
    const int* ci;
    const double* va;
    const double* rhs;   // N x W interleaved
    double* d;           // N x W interleaved
    double* work;        // 4 N doubles per column
    double tol;
    long long maxit;
    int precd;
};

template <int W>
__global__ __launch_bounds__(BT) void k_blk_pcg(BlkPcgArgs a) {
    __shared__ double red[16];
    const int col = blockIdx.x;
    const int tid = threadIdx.x;
    const int N = a.N, L = a.L, gpb = BT / L;
    const int g = tid / L, gl = tid - g * L;
    double* r = a.work + (size_t)col * 4 * N;
    double* p = r + N;
    double* q = r + 2 * (size_t)N;
    double* dg = r + 3 * (size_t)N;
    const double* rhs = a.rhs + col;
    double* d = a.d + col;
    const int niter = (N + gpb - 1) / gpb;
    double acc = 0.0;
    for (int it = 0; it < niter; ++it) {   // r = rhs ; diag ; p = M^-1 r ; r'p     :68-70
        const int row = it * gpb + g;
        const bool valid = row < N;
        double dd = 0.0;
        if (valid)
            for (int t = a.rp[row] + gl; t < a.rp[row + 1]; t += L)
                if (a.ci[t] == row) dd = a.va[t];
        dd = group_sum(dd, L, red);
        if (valid && gl == 0) {
            const double ri = rhs[(size_t)row * W];
            const double pi = a.precd == 2 ? ri / dd : ri;
            r[row] = ri;
            dg[row] = dd;
            p[row] = pi;
            d[(size_t)row * W] = 0.0;
            acc += ri * pi;
        }
    }
    double delta_new = block_sum(acc, red);
    const double delta_0 = delta_new;
    const double thresh = a.tol * a.tol * delta_0;
    long long it_count = 0;
    while (it_count < a.maxit && delta_new > thresh) {                          // :76
        const double delta_old = delta_new;
        __syncthreads();
        acc = 0.0;
        for (int it = 0; it < niter; ++it) {   // q = H p ; q'p
            const int row = it * gpb + g;
            const bool valid = row < N;
            double s = 0.0;
            if (valid)
                for (int t = a.rp[row] + gl; t < a.rp[row + 1]; t += L) s += a.va[t] * p[a.ci[t]];
            s = group_sum(s, L, red);
            if (valid && gl == 0) {
                q[row] = s;
                acc += s * p[row];
            }
        }
        const double qp = block_sum(acc, red);
        const double alpha = delta_old / qp;                                    // :78
        acc = 0.0;
        for (int row = tid; row < N; row += BT) {
            double* dr = d + (size_t)row * W;
            *dr = *dr + alpha * p[row];
            const double ri = r[row] - alpha * q[row];                          // :79
            r[row] = ri;
            const double wi = a.precd == 2 ? ri / dg[row] : ri;                 // :80
            q[row] = wi;
            acc += ri * wi;
        }
        delta_new = block_sum(acc, red);                                        // :81
        const double beta = delta_new / delta_old;                              // :82
        for (int row = tid; row < N; row += BT) p[row] = q[row] + beta * p[row];  // :83
        ++it_count;
    }
}

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

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// (ipd_block_state.h)
BlockState* block_state(ipd_amg* h, int W) {
    if (!h->blk) h->blk = std::make_shared<BlockState>();
    BlockState* bs = h->blk.get();
    IPD_REQUIRE(amg_block_levels(h, &bs->lv), IPD_E_ARG, "solve_multi: the hierarchy is sharded over ranks");
    if (bs->W >= W) return bs;
    // (re)made for the wider block out of the hierarchy's own storage: never the per-call zero pool
    Arena& ar = *h->arena;
    bs->v.assign((size_t)h->J + 1, BlockVecs{});
    for (int k = 1; k <= h->J; ++k) {
        const size_t n = (size_t)bs->lv[(size_t)k].N * W;
        BlockVecs& bv = bs->v[(size_t)k];
        bv.r = ar.alloc<double>(n);
        bv.e = ar.alloc<double>(n);
        bv.e2 = ar.alloc<double>(n);
        bv.w = ar.alloc<double>(n);
        bv.rr = ar.alloc<double>(n);
    }
    const size_t n1 = (size_t)bs->lv[1].N * W;
    bs->x[0] = ar.alloc<double>(n1);
    bs->x[1] = ar.alloc<double>(n1);
    bs->b = ar.alloc<double>(n1);
    bs->hist = ar.alloc<double>((size_t)HB * BLK_WMAX);
    bs->pcg_work = ar.alloc<double>(4 * (size_t)bs->lv[(size_t)h->J].N * W);
    bs->W = W;
    return bs;
}

void block_in(ipd_ctx* ctx, int N, int W, int ncol, const double* src, long long ld, double* dst) {
    hipLaunchKernelGGL(k_blk_in, dim3(block_io_grid(N, W)), dim3(BLK_IO_BT), 0, ctx->stream, N, W, ncol, src, ld,
                       dst);
    IPD_KERNEL_CHECK();
}

void block_out(ipd_ctx* ctx, int N, int W, int ncol, const double* src, double* dst, long long ld) {
    hipLaunchKernelGGL(k_blk_out, dim3(block_io_grid(N, W)), dim3(BLK_IO_BT), 0, ctx->stream, N, W, ncol, src, dst,
                       ld);
    IPD_KERNEL_CHECK();
}

// one launch of a <W, STAGED> kernel
#define BLK_GO(KERNEL, W, st, grid, args)                                                                  \
    do {                                                                                                   \
        if (st.staged)                                                                                     \
            hipLaunchKernelGGL((KERNEL<W, true>), dim3(grid), dim3(BT), st.dyn, ctx->stream, args);        \
        else                                                                                               \
            hipLaunchKernelGGL((KERNEL<W, false>), dim3(grid), dim3(BT), 0, ctx->stream, args);            \
        IPD_KERNEL_CHECK();                                                                                \
    } while (0)

template <int W>
struct BlockRun {
    ipd_amg* h;
    ipd_ctx* ctx;
    BlockState* bs;

    void sweep(int k, bool post) {   // launch_sweep (ipd_cycle.hip), CSR form
        const BlockLevel& bl = bs->lv[(size_t)k];
        BlockVecs& v = bs->v[(size_t)k];
        BlkSmoothArgs a;
        a.rp = bl.A.rp;
        a.ci = bl.A.ci;
        a.va = bl.A.va;
        a.N = bl.N;
        a.L = bl.A.L;
        a.r = v.r;
        a.dinv = bl.dinv;
        a.Axi = bl.Axi;
        a.xx = bl.xx;
        a.eold = v.e;
        a.win = v.w;
        a.enew = v.e2;
        a.wout = v.w;
        a.isnsp = h->opts.isnsp;
        a.eold_zero = v.e_zero ? 1 : 0;
        const BlockStage st = block_stage(bl.N, W);
        const HalfRanges& hr = bl.sweep[post ? 1 : 0];   // the ranges and the protocol of launch_sweep
        a.u0 = a.u1 = 0;
        for (int i = 0; i < hr.n; ++i) {
            if (i == hr.n - 1) a.wout = nullptr;
            a.row0 = hr.r[i].r0;
            a.row1 = hr.r[i].r1;
            BLK_GO(k_blk_smooth, W, st, hr.r[i].G, a);
            a.u0 = a.row0;
            a.u1 = a.row1;
        }
        v.e_zero = false;
        std::swap(v.e, v.e2);
    }

    // y = x2 - M x (residual, x2 = r) or y = M x / y += M x (transfers, x2 = NULL)
    void walk(const BlockCsr& m, const double* x, const double* x2, double* y, int add) {
        BlkWalkArgs a{};
        a.rp = m.rp;
        a.ci = m.ci;
        a.va = m.va;
        a.L = m.L;
        a.nrows = m.nr;
        a.ncols = m.nc;
        a.x = x;
        a.x2 = x2;
        a.y = y;
        a.add = add;
        const BlockStage st = block_stage(m.nc, W);
        if (x2)
            BLK_GO(k_blk_resid, W, st, m.grid, a);
        else
            BLK_GO(k_blk_xfer, W, st, m.grid, a);
    }

    // amg_cycle (ipd_cycle.hip): A_k e = r_k on the block; keep_e: start from the current e
    void cycle(int k, bool wc, bool keep_e) {
        const BlockLevel& bl = bs->lv[(size_t)k];
        BlockVecs& v = bs->v[(size_t)k];
        if (k == h->J) {                                                          // MG_Vcycle.m:43
            BlkPcgArgs a;
            a.N = bl.N;
            a.L = bl.pcg_L;
            a.rp = bl.A.rp;
            a.ci = bl.A.ci;
            a.va = bl.A.va;
            a.rhs = v.r;
            a.d = v.e;
            a.work = bs->pcg_work;
            a.tol = bl.pcg_tol;
            a.maxit = bl.pcg_maxit;
            a.precd = bl.pcg_precd;
            hipLaunchKernelGGL(k_blk_pcg<W>, dim3(W), dim3(BT), 0, ctx->stream, a);
            IPD_KERNEL_CHECK();
            v.e_zero = false;
            return;
        }
        const int nu = h->opts.smoth;
        if (!keep_e) {
            v.e_zero = true;
            if (nu == 0) {   // no sweep will overwrite the iterate: materialise the zero
                IPD_HIP(hipMemsetAsync(v.e, 0, sizeof(double) * (size_t)bl.N * W, ctx->stream));
                v.e_zero = false;
            }
        }
        for (int s = 0; s < nu; ++s) sweep(k, false);                            // :14-25
        BlockVecs& cv = bs->v[(size_t)k + 1];
        if (bl.T1.rp) {   // r_{k+1} = P'r - (P'A) e                                 :27
            BlkWalkArgs a{};
            a.rp = bl.Pt.rp;
            a.ci = bl.Pt.ci;
            a.va = bl.Pt.va;
            a.rp2 = bl.T1.rp;
            a.ci2 = bl.T1.ci;
            a.va2 = bl.T1.va;
            a.L = bl.T1.L;
            a.nrows = bl.Pt.nr;
            a.ncols = bl.Pt.nc;
            a.x = v.r;
            a.x2 = v.e;
            a.y = cv.r;
            const BlockStage st = block_stage(2LL * bl.Pt.nc, W);   // r and e of the fine level
            BLK_GO(k_blk_rrc, W, st, bl.T1.grid, a);
        } else {
            walk(bl.A, v.e, v.r, v.rr, 0);                                    // rr = r - A e
            walk(bl.Pt, v.rr, nullptr, cv.r, 0);                              // r_{k+1} = P' rr
        }
        cycle(k + 1, wc, false);                                                 // :29
        if (wc && k + 1 < h->J) cycle(k + 1, wc, true);                          // MG_Wcycle.m:30
        walk(bl.P, cv.e, nullptr, v.e, 1);                                    // e += P e_{k+1}  :31
        for (int s = 0; s < nu; ++s) sweep(k, true);                             // :33-41
    }

    void top(const double* x, const double* e, double* xnew, bool first) {
        const BlockLevel& bl = bs->lv[1];
        BlkWalkArgs a{};
        a.rp = bl.A.rp;
        a.ci = bl.A.ci;
        a.va = bl.A.va;
        a.L = bl.A.L;
        a.nrows = bl.N;
        a.ncols = bl.N;
        a.x = x;
        a.x2 = e;
        a.b = bs->b;
        a.y = bs->v[1].r;
        a.y2 = xnew;
        a.hist = first ? nullptr : bs->hist;
        const BlockStage st = block_stage(bl.N, W);
        BLK_GO(k_blk_top, W, st, bl.A.grid, a);
        const AmgOpts& o = h->opts;
        hipLaunchKernelGGL(k_blk_conv<W>, dim3(1), dim3(BT), 0, ctx->stream, (const double*)bs->v[1].r, bl.N,
                           bs->hist, first ? 1 : 0, o.retol, (double)o.maxit);
        IPD_KERNEL_CHECK();
    }

    // Class_AMG.m:86-109 for the columns j0 .. j0+ncol-1 of the call
    void solve(const double* B, long long ldb, int ncol, const double* guess, double* X, int32_t* it,
               double* rel_res, double* rel_resk, double* rhok) {
        const AmgOpts& o = h->opts;
        const int N = bs->lv[1].N;
        block_in(ctx, N, W, ncol, B, ldb, bs->b);
        block_in(ctx, N, W, ncol, guess, ldb, bs->x[0]);
        int cur = 0;
        top(bs->x[0], nullptr, bs->x[1], true);                                   // :89
        cur = 1;
        std::vector<double> hh((size_t)HB * W);
        ctx->fetch(bs->hist, hh.data(), hh.size());
        const long long hs = multi_hist_stride(o.maxit);
        std::vector<int> cnt((size_t)ncol, 0);
        bool any = false;
        for (int c = 0; c < ncol; ++c) {
            const double* H = hh.data() + (size_t)c * HB;
            double* rk = rel_resk ? rel_resk + c * hs : nullptr;
            double* rh = rhok ? rhok + c * hs : nullptr;
            if (H[HB_RES0] == 0.0) {                                              // :91-92
                if (rk) rk[0] = 0.0;
                if (rh) rh[0] = INFINITY;
            } else {                                                              // :94
                if (rk) rk[0] = 1.0;
                if (rh) rh[0] = NAN;
            }
            rel_res[c] = 0.0;
            any = any || H[HB_ACT] != 0.0;
        }
        const bool wc = o.cycle == 'w', vc = o.cycle == 'v';
        while (any) {                                                             // :95
            const double* e = nullptr;
            if (vc || wc) {
                cycle(1, wc, false);                                              // :96-102
                e = bs->v[1].e;
            }
            top(bs->x[cur], e, bs->x[cur ^ 1], false);                            // :103-105
            cur ^= 1;
            ctx->fetch(bs->hist, hh.data(), hh.size());
            any = false;
            for (int c = 0; c < ncol; ++c) {
                const double* H = hh.data() + (size_t)c * HB;
                const int n = (int)H[HB_CNT];
                if (n > cnt[(size_t)c]) {
                    cnt[(size_t)c] = n;
                    if (rel_resk) rel_resk[c * hs + n] = H[HB_REL];
                    if (rhok) rhok[c * hs + n] = H[HB_RHO];
                    rel_res[c] = H[HB_REL];
                }
                any = any || H[HB_ACT] != 0.0;
            }
        }
        for (int c = 0; c < ncol; ++c) it[c] = cnt[(size_t)c];                    // :108
        block_out(ctx, N, W, ncol, bs->x[cur], X, ldb);
        ctx->sync();
    }
};

// run(BlockRun<W>) for the run-time width W
template <class F>
static void with_block_run(ipd_amg* h, BlockState* bs, int W, F&& run) {
    with_block_width(W, [&](auto Wc) { run(BlockRun<decltype(Wc)::value>{h, h->ctx, bs}); });
}

// (ipd_block_state.h)
void block_cycle(ipd_amg* h, BlockState* bs, int W, bool wc) {
    with_block_run(h, bs, W, [&](auto run) { run.cycle(1, wc, false); });
}

// all columns, in chunks of at most BLK_WMAX (device B, guess, X; host outputs)
static void amg_solve_multi_dev(ipd_amg* h, const double* B, long long ldb, long long nrhs, const double* guess,
                                double* X, int32_t* it, double* rel_res, double* rel_resk, double* rhok) {
    const long long hs = multi_hist_stride(h->opts.maxit);
    std::vector<double> rr((size_t)nrhs);
    block_chunks(nrhs, [&](long long j0, int ncol, int W) {
        with_block_run(h, block_state(h, W), W, [&](auto run) {
            run.solve(B + j0 * ldb, ldb, ncol, guess ? guess + j0 * ldb : nullptr, X + j0 * ldb, it + j0,
                      rr.data() + j0, rel_resk ? rel_resk + j0 * hs : nullptr, rhok ? rhok + j0 * hs : nullptr);
        });
    });
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
        CallScope scope(h->ctx);
        block_host_call(h, B, ldb, nrhs, guess, X, [&](const double* dB, const double* dg, double* dX) {
            amg_solve_multi_dev(h, dB, ldb, nrhs, dg, dX, it, rel_res, rel_resk, rhok);
        });
    });
}
