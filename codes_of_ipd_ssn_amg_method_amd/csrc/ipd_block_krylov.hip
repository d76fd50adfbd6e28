// AMG-preconditioned conjugate gradients for several right-hand sides through one hierarchy: column j
// of E runs the loop of ipd_amg_pcg (ipd_krylov.hip; PCG.m:68-87, M = one cycle from a zero guess,
// flexible beta) as if it were solved alone, every column of a block in lockstep.
//
// The vectors are the block path's: N x W row-major, W in {1, 2, 4, 8}, block_in / block_out at the
// edges, and the preconditioner is block_cycle on the CSR arrays of every level (ipd_block_state.h: this
// unit instantiates and launches the k_bkry_* kernels only; the row-walk helpers are ipd_block_dev.h's).
// One iteration is the block form of ipd_krylov.hip's four steps and one host read of the W x SC_N scalar
// records:
//   K1 k_bkry_dir_spmv  p_new(:,c) = w(:,c) + beta_c p_old(:,c) formed inside the level-1 CSR row
//                       walk's gather (p_old is only read), p_new and w_old stored for the owned rows,
//                       q = A_1 p_new for all W columns (each matrix entry read once), per-workgroup
//                       partials of p_new(:,c)'q(:,c); the last workgroup forms every alpha_c.  With
//                       START it forms r = E - A_1 D0 instead.
//   K2 k_bkry_update    active columns: D += alpha_c p ; r -= alpha_c q.  The new r goes into the block
//                       cycle's input v[1].r, zero for a frozen column (which then gets e = 0).
//   cycle               block_cycle: w = v[1].e.
//   K3 k_bkry_dots      r'w and r'w_old per column in one pass; the last workgroup takes the step of
//                       ipd_pcg_step.h for every active column, and forms the "any active" word.
// Frozen columns: a column whose stop flag is set keeps D, r and its record; K1 gathers zero for it.
// Padding columns are zero and stop at the first test (delta_0 = 0).
// Reductions: per-workgroup partials, one row of G per column, summed in fixed workgroup order by the
// workgroup that arrives last (kry_last_arrival / kry_sum_parts): no float atomics, the same bits run
// to run, and no column's sum sees another column's data.  Separate multiplies and adds.
#include "ipd_block_state.h"

#include "ipd_block_dev.h"
#include "ipd_krylov.h"

struct BlockKrylovState {
    int W = 0;                   // width the vectors were made for
    int N = 0;
    int G1 = 0, G3 = 0;          // workgroups of K1 / of K2 and K3
    double* p[2] = {nullptr, nullptr};   // p[0] also holds the guess block until the first direction
    double* q = nullptr;
    double* w_old = nullptr;
    double* d = nullptr;
    double* r = nullptr;
    double* e = nullptr;         // right-hand sides
    double* sc = nullptr;        // SC_N x W records, then the "any active" word
    double* part1 = nullptr;     // W x G1 partials of p'q
    double* part3 = nullptr;     // 2W x G3 partials of r'w, r'w_old
    unsigned* cnt = nullptr;     // tickets of K1 and K3
};

struct BkryDirArgs {
    const int* rp;
    const int* ci;
    const double* va;
    int N, L;
    const double* w;       // preconditioned residuals; START: the guess block
    const double* p_old;   // NULL: first direction (beta = 0, p_old not read)
    double* p_new;
    double* w_old;
    double* q;
    const double* e;       // START: right-hand sides
    double* r;             // START: residuals (the PCG's copy) ...
    double* r1;            // ... and the block cycle's input v[1].r
    double* d;             // START: D = D0
    double* sc;
    double* part;
    unsigned* cnt;
};

// bit c: column c has not stopped
template <int W>
__device__ __forceinline__ unsigned bkry_active(const double* sc) {
    unsigned act = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) act |= sc[c * SC_N + SC_STOP] == 0.0 ? 1u << c : 0u;
    return act;
}

// the workgroup's sums of v[c] into part[c * gridDim.x + blockIdx.x], c < W, in a fixed order (wave sums,
// then waves 0..BLK_WAVES-1); threads c < W (wave 0) store them.  Unlike blk_block_sum, only the storing
// threads read the W x BLK_WAVES wave sums back (all threads holding them took 128 VGPRs at W = 8).
template <int W>
__device__ __forceinline__ void bkry_block_parts(double (&v)[W], double* red, double* part) {
    const int w = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = wave_sum(v[c]);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) red[c * BLK_WAVES + w] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < W) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < BLK_WAVES; ++k) t += red[threadIdx.x * BLK_WAVES + k];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

template <int W, bool STAGED, bool START>
__global__ __launch_bounds__(BT) void k_bkry_dir_spmv(BkryDirArgs a) {
    __shared__ double red[W * BLK_WAVES];
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const double* __restrict__ w = a.w;
    const double* __restrict__ po = a.p_old;
    // beta_c per column, kept in LDS (W uniform values would take SGPRs)
    __shared__ __attribute__((aligned(16))) double bsh[W];
    const unsigned act = START ? (1u << W) - 1u : bkry_active<W>(a.sc);
    if (threadIdx.x < W) bsh[threadIdx.x] = (!START && po) ? a.sc[threadIdx.x * SC_N + SC_BETA] : 0.0;
    __syncthreads();
    auto gather = [&](int j, double (&y)[W]) {
        blk_load<W>(w + (size_t)j * W, y);
        if (START) return;
        double pv[W], bv[W];
        if (po) {
            blk_load<W>(po + (size_t)j * W, pv);
            blk_load<W>(bsh, bv);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) y[c] = (act >> c & 1u) ? (po ? y[c] + bv[c] * pv[c] : y[c]) : 0.0;
    };
    double acc[W];
#pragma unroll
    for (int c = 0; c < W; ++c) acc[c] = 0.0;
    auto epi = [&](int row, const double (&s)[W]) {
        double xo[W];
        if (STAGED)
            blk_load<W>(xs + (size_t)row * W, xo);
        else
            gather(row, xo);
        if (START) {                                                              // PCG.m:68
            double ev[W], rv[W];
            blk_load<W>(a.e + (size_t)row * W, ev);
#pragma unroll
            for (int c = 0; c < W; ++c) rv[c] = ev[c] - s[c];
            blk_store<W>(a.r + (size_t)row * W, rv);
            blk_store<W>(a.r1 + (size_t)row * W, rv);
            blk_store<W>(a.d + (size_t)row * W, xo);
        } else {
            double wv[W];
            blk_load<W>(w + (size_t)row * W, wv);
            blk_store<W>(a.p_new + (size_t)row * W, xo);
            blk_store<W>(a.w_old + (size_t)row * W, wv);
            blk_store<W>(a.q + (size_t)row * W, s);                               // :77
#pragma unroll
            for (int c = 0; c < W; ++c) acc[c] += xo[c] * s[c];
        }
    };
    blk_walk<W, STAGED>(a.rp, a.ci, a.va, a.L, a.N, 0, a.N, true, gather, epi, red, xs);
    if (START) return;
    const int G = gridDim.x;
    bkry_block_parts<W>(acc, red, a.part);
    if (threadIdx.x >= 64 || !kry_last_arrival(a.cnt)) return;
    // one column at a time: unrolled, W = 8 without staging spilled SGPRs
#pragma unroll 1
    for (int c = 0; c < W; ++c) {
        const double pq = kry_sum_parts(a.part + (size_t)c * G, G, 1);
        if (threadIdx.x == 0 && (act >> c & 1u)) pcg_step_alpha(a.sc + c * SC_N, pq);   // :77-78
    }
}

// active columns: D += alpha p ; r -= alpha q.  v[1].r = r (frozen columns: 0)          PCG.m:79
template <int W>
__global__ __launch_bounds__(BT) void k_bkry_update(int N, const double* __restrict__ sc,
                                                    const double* __restrict__ p, const double* __restrict__ q,
                                                    double* __restrict__ d, double* __restrict__ r,
                                                    double* __restrict__ r1) {
    const unsigned act = bkry_active<W>(sc);
    for (int i = blockIdx.x * BT + threadIdx.x; i < N; i += gridDim.x * BT) {
        const size_t o = (size_t)i * W;
        double pv[W], qv[W], dv[W], rv[W], r1v[W];
        blk_load<W>(p + o, pv);
        blk_load<W>(q + o, qv);
        blk_load<W>(d + o, dv);
        blk_load<W>(r + o, rv);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const bool on = act >> c & 1u;
            const double alpha = sc[c * SC_N + SC_ALPHA];
            dv[c] = on ? dv[c] + alpha * pv[c] : dv[c];
            rv[c] = on ? rv[c] - alpha * qv[c] : rv[c];
            r1v[c] = on ? rv[c] : 0.0;
        }
        blk_store<W>(d + o, dv);
        blk_store<W>(r + o, rv);
        blk_store<W>(r1 + o, r1v);
    }
}

struct BkryDotArgs {
    int N;
    const double* r;
    const double* w;
    const double* w_old;   // FIRST: not read
    double tol2;           // retol^2
    double maxit;
    double* sc;
    double* part;          // [r'w of columns 0..W-1 | r'w_old of columns 0..W-1] x G
    unsigned* cnt;
};

template <int W, bool FIRST>
__global__ __launch_bounds__(BT) void k_bkry_dots(BkryDotArgs a) {
    __shared__ double red[W * BLK_WAVES];
    const int G = gridDim.x, b = blockIdx.x;
    double rw[W], rwo[W];
#pragma unroll
    for (int c = 0; c < W; ++c) rw[c] = rwo[c] = 0.0;
    for (int i = b * BT + threadIdx.x; i < a.N; i += G * BT) {
        double rv[W], wv[W];
        blk_load<W>(a.r + (size_t)i * W, rv);
        blk_load<W>(a.w + (size_t)i * W, wv);
#pragma unroll
        for (int c = 0; c < W; ++c) rw[c] += rv[c] * wv[c];
        if (!FIRST) {
            blk_load<W>(a.w_old + (size_t)i * W, wv);
#pragma unroll
            for (int c = 0; c < W; ++c) rwo[c] += rv[c] * wv[c];
        }
    }
    bkry_block_parts<W>(rw, red, a.part);
    if (!FIRST) bkry_block_parts<W>(rwo, red, a.part + (size_t)W * G);
    if (threadIdx.x >= 64 || !kry_last_arrival(a.cnt)) return;
    const unsigned act = FIRST ? (1u << W) - 1u : bkry_active<W>(a.sc);
    bool any = false;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const double dn = kry_sum_parts(a.part + (size_t)c * G, G, 1);
        const double s_wo = FIRST ? 0.0 : kry_sum_parts(a.part + (size_t)(W + c) * G, G, 1);
        if (threadIdx.x == 0 && (act >> c & 1u)) {                                // PCG.m:70-72, :81-85, :76
            const bool go = pcg_step<FIRST>(a.sc + c * SC_N, dn, s_wo, a.maxit, a.tol2);
            any = any || go;
        }
    }
    if (threadIdx.x == 0) a.sc[W * SC_N] = any ? 1.0 : 0.0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static BlockKrylovState* bkry_state(ipd_amg* h, int W, int N, int G1, int G3) {
    if (!h->bkry) h->bkry = std::make_shared<BlockKrylovState>();
    BlockKrylovState* ks = h->bkry.get();
    if (ks->W >= W) {
        IPD_REQUIRE(ks->N == N && ks->G1 == G1 && ks->G3 == G3, IPD_E_ARG,
                    "AMG-PCG multi: level-1 geometry changed");
        return ks;
    }
    // (re)made for the wider block out of the hierarchy's own storage: never the per-call zero pool
    Arena& ar = *h->arena;
    const size_t n = (size_t)N * W;
    for (auto& v : ks->p) v = ar.alloc<double>(n);
    ks->q = ar.alloc<double>(n);
    ks->w_old = ar.alloc<double>(n);
    ks->d = ar.alloc<double>(n);
    ks->r = ar.alloc<double>(n);
    ks->e = ar.alloc<double>(n);
    ks->sc = ar.alloc<double>((size_t)SC_N * W + 1);
    ks->part1 = ar.alloc<double>((size_t)G1 * W);
    ks->part3 = ar.alloc<double>(2 * (size_t)G3 * W);
    ks->cnt = ar.alloc<unsigned>(2);
    ks->W = W;
    ks->N = N;
    ks->G1 = G1;
    ks->G3 = G3;
    return ks;
}

#define BKRY_K1(W, START, args)                                                                             \
    do {                                                                                                    \
        if (st.staged)                                                                                      \
            hipLaunchKernelGGL((k_bkry_dir_spmv<W, true, START>), dim3(G1), dim3(BT), st.dyn, ctx->stream, args); \
        else                                                                                                \
            hipLaunchKernelGGL((k_bkry_dir_spmv<W, false, START>), dim3(G1), dim3(BT), 0, ctx->stream, args); \
        IPD_KERNEL_CHECK();                                                                                 \
    } while (0)

// the columns j0 .. j0+ncol-1 of the call (device E, guess, D; host it, res, resk)
template <int W>
static void pcg_chunk(ipd_amg* h, const double* E, long long lde, int ncol, const double* guess, double tol,
                      long long maxit, double* D, int64_t* it, double* res, double* resk) {
    ipd_ctx* ctx = h->ctx;
    BlockState* bs = block_state(h, W);
    const BlockLevel& bl = bs->lv[1];
    const int N = bl.N;
    const int G1 = bl.A.grid;
    const int G3 = krylov_g3(N, ctx->num_cu);
    BlockKrylovState* ks = bkry_state(h, W, N, G1, G3);
    const BlockStage st = block_stage(N, W);
    const bool wc = h->opts.cycle == 'w';
    double* r1 = bs->v[1].r;
    block_in(ctx, N, W, ncol, E, lde, ks->e);
    block_in(ctx, N, W, ncol, guess, lde, ks->p[0]);
    // tickets start at zero on every call (the last arriver resets its own, this covers a launch
    // that never completed)
    IPD_HIP(hipMemsetAsync(ks->cnt, 0, 2 * sizeof(unsigned), ctx->stream));

    BkryDirArgs walk{};   // level 1's row walk, for both forms of K1
    walk.rp = bl.A.rp;
    walk.ci = bl.A.ci;
    walk.va = bl.A.va;
    walk.N = N;
    walk.L = bl.A.L;
    BkryDirArgs ka = walk;
    ka.w = ks->p[0];                                                              // PCG.m:68
    ka.e = ks->e;
    ka.r = ks->r;
    ka.r1 = r1;
    ka.d = ks->d;
    BKRY_K1(W, true, ka);
    BkryDotArgs kd{};
    kd.N = N;
    kd.r = ks->r;
    kd.w_old = ks->w_old;
    kd.tol2 = tol * tol;
    kd.maxit = (double)maxit;
    kd.sc = ks->sc;
    kd.part = ks->part3;
    kd.cnt = ks->cnt + 1;
    block_cycle(h, bs, W, wc);                                                     // :69
    kd.w = bs->v[1].e;
    hipLaunchKernelGGL((k_bkry_dots<W, true>), dim3(G3), dim3(BT), 0, ctx->stream, kd);
    IPD_KERNEL_CHECK();
    std::vector<double> sc((size_t)SC_N * W + 1);
    ctx->fetch(ks->sc, sc.data(), sc.size());
    std::vector<char> act((size_t)ncol);
    for (int c = 0; c < ncol; ++c) {
        it[c] = 0;
        act[(size_t)c] = sc[(size_t)c * SC_N + SC_STOP] == 0.0;
    }

    ka = walk;
    ka.w_old = ks->w_old;
    ka.q = ks->q;
    ka.sc = ks->sc;
    ka.part = ks->part1;
    ka.cnt = ks->cnt;
    int cur = 0;   // p[cur]: the current directions
    bool have_p = false;
    while (sc[(size_t)SC_N * W] != 0.0) {                                         // :76, any column
        ka.w = bs->v[1].e;
        ka.p_old = have_p ? ks->p[cur] : nullptr;
        ka.p_new = ks->p[cur ^ 1];
        BKRY_K1(W, false, ka);                                                    // :77-78, :83
        cur ^= 1;
        have_p = true;
        hipLaunchKernelGGL(k_bkry_update<W>, dim3(G3), dim3(BT), 0, ctx->stream, N, (const double*)ks->sc,
                           (const double*)ks->p[cur], (const double*)ks->q, ks->d, ks->r, r1);
        IPD_KERNEL_CHECK();                                                       // :79
        block_cycle(h, bs, W, wc);                                                 // :80
        kd.w = bs->v[1].e;
        hipLaunchKernelGGL((k_bkry_dots<W, false>), dim3(G3), dim3(BT), 0, ctx->stream, kd);
        IPD_KERNEL_CHECK();                                                       // :81-82, :84-85
        ctx->fetch(ks->sc, sc.data(), sc.size());
        for (int c = 0; c < ncol; ++c) {
            if (!act[(size_t)c]) continue;
            const double* S = sc.data() + (size_t)c * SC_N;
            it[c] = (int64_t)S[SC_IT];
            if (resk) resk[pcg_resk_slot(c, maxit, it[c])] = S[SC_RES];
            act[(size_t)c] = S[SC_STOP] == 0.0;
        }
    }
    if (res)
        for (int c = 0; c < ncol; ++c) res[c] = sc[(size_t)c * SC_N + SC_RES];   // :88
    block_out(ctx, N, W, ncol, ks->d, D, lde);
    ctx->sync();
}

// all columns, in chunks of at most BLK_WMAX (device E, guess, D; host outputs)
static void amg_pcg_multi_dev(ipd_amg* h, const double* E, long long lde, long long nrhs, const double* guess,
                              double tol, long long maxit, double* D, int64_t* it, double* res, double* resk) {
    block_chunks(nrhs, [&](long long j0, int ncol, int W) {
        with_block_width(W, [&](auto Wc) {
            pcg_chunk<decltype(Wc)::value>(h, E + j0 * lde, lde, ncol, guess ? guess + j0 * lde : nullptr, tol, maxit,
                                           D + j0 * lde, it + j0, res ? res + j0 : nullptr,
                                           resk ? resk + pcg_resk_slot(j0, maxit, 1) : nullptr);   // column j0's
        });
    });
}

static void check_pcg_multi_args(ipd_amg* h, const double* E, long long lde, long long nrhs, const double* D,
                                 const int64_t* it) {
    IPD_REQUIRE(h && E && D && it, IPD_E_ARG, "NULL argument");
    IPD_REQUIRE(nrhs >= 1, IPD_E_ARG, "AMG-PCG multi: nrhs must be at least 1");
    IPD_REQUIRE(lde >= (long long)h->L[1].A.nr, IPD_E_ARG, "AMG-PCG multi: lde must be at least N");
    IPD_REQUIRE(amg_block_levels(h, nullptr), IPD_E_ARG, "AMG-PCG multi: the hierarchy is sharded over ranks");
    const int cyc = h->opts.cycle;
    IPD_REQUIRE(cyc == 'v' || cyc == 'w', IPD_E_ARG,
                "AMG-PCG multi: the hierarchy's cycle must be 'v' or 'w' (any other value applies no correction)");
}

extern "C" int ipd_amg_pcg_multi_dev(ipd_amg* h, const double* E, int64_t lde, int64_t nrhs, const double* guess,
                                     const ipd_pcg_opts* o, double* D, int64_t* it, double* res, double* resk) {
    return ipd_guard([&] {
        check_pcg_multi_args(h, E, lde, nrhs, D, it);
        double tol;
        long long maxit;
        pcg_opts_of(o, &tol, &maxit);
        CallScope scope(h->ctx);
        amg_pcg_multi_dev(h, E, lde, nrhs, guess, tol, maxit, D, it, res, resk);
    });
}

extern "C" int ipd_amg_pcg_multi(ipd_amg* h, const double* E, int64_t lde, int64_t nrhs, const double* guess,
                                 const ipd_pcg_opts* o, double* D, int64_t* it, double* res, double* resk) {
    return ipd_guard([&] {
        check_pcg_multi_args(h, E, lde, nrhs, D, it);
        double tol;
        long long maxit;
        pcg_opts_of(o, &tol, &maxit);
        CallScope scope(h->ctx);
        block_host_call(h, E, lde, nrhs, guess, D, [&](const double* dE, const double* dg, double* dD) {
            amg_pcg_multi_dev(h, dE, lde, nrhs, dg, tol, maxit, dD, it, res, resk);
        });
    });
}
