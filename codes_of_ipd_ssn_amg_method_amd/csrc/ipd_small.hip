// The single-workgroup kernels -- the whole Class_AMG solve, the whole AMG-PCG solve and the sub-cycle rooted below
// the launches -- and their launches.  They run the interpreter of ipd_interp.h on an LDS image that ipd_image.hip
// has packed; this is the only unit of the cycle's host side that compiles the interpreter.
#include "ipd_cycle_state.h"

#include <cmath>

#include "ipd_interp.h"   // and ipd_cycle_pcg.h
#include "ipd_pcg_step.h"

// out[0] = it, out[1] = rel_res, out[2] = res0; rel_resk at out[4 ..], rhok at out[4+maxit+2 ..]
// fixed_cycles > 0: run exactly that many loop bodies without the stopping rules (bench hook)
template <bool CACHED>
__global__ __launch_bounds__(BT) void k_solve_small(const SolveDesc* __restrict__ D_global,
                                                    const double* __restrict__ b, double* xa,
                                                    double* xb, double* hist, double* out,
                                                    int fixed_cycles) {
    __shared__ PhaseLds lds;
    __shared__ double red[16];
    __shared__ double blkpart[48 + SOLVE_ML + 1];
    extern __shared__ __attribute__((aligned(16))) char dyn_raw[];
    // dynamic LDS: [ staging vector | descriptor copy | cached levels ]
    const SolveDesc* D = D_global;
    SolveDesc* LD = nullptr;
    if (CACHED) LD = sol_load_image(D_global, dyn_raw);
    // without cached levels the descriptor stays in global memory: its (uniform) fields
    // are then fetched with scalar loads and live in SGPRs instead of VGPRs
    SolveCtx c = sol_ctx(CACHED ? LD : D_global, &lds, red, blkpart, dyn_raw, nullptr);
    D = c.D;
    const int N = D->L[1].lv.N;
    const int maxit = D->maxit;
    double* const x_home = xa;
    double* relk = out + 4;
    double* rhok = out + 4 + (maxit + 2);
    sol_top(c, b, xa, nullptr, xb, hist, 1);                              // Class_AMG.m:89
    {
        double* t = xa;
        xa = xb;
        xb = t;
    }
    const double res0 = hist[0];
    int it = 0;
    double rel_res = 0.0;
    if (fixed_cycles > 0) {
        for (int cyc = 0; cyc < fixed_cycles; ++cyc) {
            const double* ecorr = nullptr;
            if (D->anycycle) {
                sol_cycle(c);
                ecorr = sol_e(c, 1);
            }
            sol_top(c, b, xa, ecorr, xb, hist, 0);
            double* t = xa;
            xa = xb;
            xb = t;
        }
        it = fixed_cycles;
        rel_res = hist[3];
    } else if (res0 == 0.0) {                                             // :91-92
        if (threadIdx.x == 0) {
            relk[0] = 0.0;
            rhok[0] = INFINITY;
        }
    } else {
        it = 1;                                                           // :94
        double last_rel = 1.0;
        if (threadIdx.x == 0) {
            relk[0] = 1.0;
            rhok[0] = NAN;
        }
        while (last_rel > D->retol && it <= maxit) {                      // :95
            const double* ecorr = nullptr;
            if (D->anycycle) {
                sol_cycle(c);                                             // :96-102
                ecorr = sol_e(c, 1);
            }
            sol_top(c, b, xa, ecorr, xb, hist, 0);                        // :103-105
            double* t = xa;
            xa = xb;
            xb = t;
            rel_res = hist[3];
            const double rho = hist[4];
            if (threadIdx.x == 0) {
                relk[it] = rel_res;
                rhok[it] = rho;
            }
            last_rel = rel_res;
            ++it;
            if (rho > 1.0) break;                                         // :106
            __syncthreads();  // hist is rewritten by the next conv_block
        }
        it -= 1;                                                          // :108
    }
    __syncthreads();
    if (xa != x_home)
        for (int i = threadIdx.x; i < N; i += BT) x_home[i] = xa[i];
    if (threadIdx.x == 0) {
        out[0] = (double)it;
        out[1] = rel_res;
        out[2] = res0;
    }
}

// ---------------------------------------------------------------------------
// whole AMG-PCG solve in ONE workgroup (ipd_amg_pcg_planned)
// ---------------------------------------------------------------------------
// The loop of ipd_krylov.hip (PCG.m:68-87, flexible beta) run by the workgroup that k_solve_small is, on
// the same SolveDesc / LDS image, with M(r) = sol_cycle(c) from a zero guess, the scalar rules those of
// ipd_pcg_step.h over values in registers: one launch and one
// read-back per solve.  The PCG's own vectors (d, r, p, q, w_old) are the hierarchy's krylov_state
// vectors in global memory (<= 8 KB each, L2-resident): the image's LDS budget is planned to the byte
// for the stationary solve, and five more level-1 vectors would push level 1 of the larger mode-1
// hierarchies out of it.  The PCG keeps its own r apart from the cycle's input L[1].lv.r.
// Reductions are block_sum's (per-thread strided partials, wave sums, the waves summed in fixed
// order, every thread reading the same total), so the loop test is uniform and the bits repeat.
struct PcgSmallArgs {
    const double* e;   // right-hand side
    double* d;         // in: initial guess, out: solution
    double* r;         // the PCG's residual
    double* p;
    double* q;
    double* w_old;
    double tol2;       // retol^2
    int maxit;
    double* out;       // out[0] = it, out[1] = res, out[2] = delta_0; resk at out[4 .. 4 + maxit)
};

// p = w + beta p (p not read for the first direction), w_old = w, q = A_1 p by the level-1 row walk
// with the gather staged in c.xs; returns the thread's share of p'q.  k_kry_dir_spmv for one workgroup.
__device__ __forceinline__ double pcgs_dir_spmv(SolveCtx& c, const PcgSmallArgs& a,
                                                const double* __restrict__ w, double beta,
                                                bool have_p) {
    const LevelDev& lv = c.D->L[1].lv;
    double* xs = c.xs;
    const int tid = threadIdx.x;
    const int N = lv.N, L = lv.L, gpb = BT / L;
    const int g = tid / L, gl = tid - g * L;
    const bool uni = L >= 64;
    const int niter = (N + gpb - 1) / gpb;
    const double* po = a.p;
    auto xlds = [&](int j) { return xs[j]; };
    int row = uniform_if(g, uni);
    bool valid = row < N;
    bool owner = valid && gl == 0;
    RowCursor rc;
    RowBatch bt;
    row_open<false>(lv, row, valid, owner, gl, L, rc, bt);
    if (have_p)
        vec_pass(N, [&](int j) { return w[j] + beta * po[j]; }, [&](int j, double v) { xs[j] = v; });
    else
        vec_pass(N, [&](int j) { return w[j]; }, [&](int j, double v) { xs[j] = v; });
    __syncthreads();   // every p_old is read before an owner stores its p_new
    double acc = 0.0;
    for (int it = 0; it < niter; ++it) {
        if (it > 0) {
            row = uniform_if(it * gpb + g, uni);
            valid = row < N;
            owner = valid && gl == 0;
            row_open<false>(lv, row, valid, owner, gl, L, rc, bt);
        }
        double s = row_finish<false>(lv, rc, bt, gl, L, xlds);
        double dummy;
        s = reduce_rows(s, L, false, 0.0, &dummy, c.lds);
        if (owner) {
            const double xo = xs[row];
            a.p[row] = xo;
            a.w_old[row] = w[row];
            a.q[row] = s;                                                     // PCG.m:77
            acc += xo * s;
        }
    }
    return acc;
}

template <bool CACHED>
__global__ __launch_bounds__(BT) void k_pcg_small(const SolveDesc* __restrict__ D_global,
                                                  const PcgSmallArgs a) {
    __shared__ PhaseLds lds;
    __shared__ double red[16];
    __shared__ double blkpart[48 + SOLVE_ML + 1];
    extern __shared__ __attribute__((aligned(16))) char dyn_raw[];
    SolveDesc* LD = nullptr;
    if (CACHED) LD = sol_load_image(D_global, dyn_raw);
    SolveCtx c = sol_ctx(CACHED ? LD : D_global, &lds, red, blkpart, dyn_raw, nullptr);
    const SolveDesc* D = c.D;
    const int N = D->L[1].lv.N;
    double* const r1 = D->L[1].lv.r;   // the cycle's input
    {   // r = e - A_1 d0 (PCG.m:68); the walk's copy of d0 goes to p, which the first direction overwrites
        TopArgs ta;
        ta.lv = D->L[1].lv;
        ta.b = a.e;
        ta.x = a.d;
        ta.e = nullptr;
        ta.xnew = a.p;
        ta.row0 = 0;
        ta.row1 = N;
        ta.staged = 1;
        phase_top<true, false>(ta, 0, 1, c.lds, c.xs);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < N; i += BT) a.r[i] = r1[i];
    __syncthreads();
    sol_cycle(c);                                                             // :69
    const double* w = sol_e(c, 1);
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += BT) acc += a.r[i] * w[i];
    double delta = block_sum(acc, red);                                       // :70
    const double delta0 = delta;
    double beta = 0.0;
    double res = pcg_res(delta, delta0);
    int it = 0;
    while (it < a.maxit && delta > a.tol2 * delta0) {   // :76, restates pcg_step's test (ipd_pcg_step.h) on an int count
        const double pq = block_sum(pcgs_dir_spmv(c, a, w, beta, it > 0), red);   // :77, :83
        const double alpha = delta / pq;                                      // :78
        for (int i = threadIdx.x; i < N; i += BT) {                           // :79
            a.d[i] = a.d[i] + alpha * a.p[i];
            const double ri = a.r[i] - alpha * a.q[i];
            a.r[i] = ri;
            r1[i] = ri;
        }
        __syncthreads();
        sol_cycle(c);                                                         // :80
        w = sol_e(c, 1);
        double rw = 0.0, rwo = 0.0;
        for (int i = threadIdx.x; i < N; i += BT) {
            const double ri = a.r[i];
            rw += ri * w[i];
            rwo += ri * a.w_old[i];
        }
        const double dn = block_sum(rw, red);                                 // :81
        const double s_wo = block_sum(rwo, red);
        beta = pcg_beta(dn, s_wo, delta);                                     // flexible :82
        delta = dn;
        ++it;                                                                 // :84
        res = pcg_res(dn, delta0);                                            // :85
        if (threadIdx.x == 0) a.out[4 + it - 1] = res;
    }
    if (threadIdx.x == 0) {
        a.out[0] = (double)it;
        a.out[1] = res;                                                       // :88
        a.out[2] = delta0;
    }
}

// Sub-cycle rooted at level k_lds >= 2 of a hierarchy whose upper levels run as multi-workgroup
// launches: ONE workgroup, every level from the root down cached in LDS.  r_{root} is read from
// and the correction written to the global vectors the surrounding launches use.
__global__ __launch_bounds__(BT) void k_subcycle(const SolveDesc* __restrict__ D_global, int keep) {
    __shared__ PhaseLds lds;
    __shared__ double red[16];
    __shared__ double blkpart[48 + SOLVE_ML + 1];
    extern __shared__ __attribute__((aligned(16))) char dyn_raw[];
    const SolveDesc* D = D_global;
    long long* dbg = D->dbg;
    if (dbg && threadIdx.x == 0) dbg[0] = wall_clock64();
    SolveDesc* LD = sol_load_image(D_global, dyn_raw);
    if (dbg && threadIdx.x == 0) dbg[1] = wall_clock64();
    const int k0 = D->k_lds, N0 = D->L[k0].lv.N;
    {
        double* r = LD->L[k0].lv.r;
        double* e = LD->L[k0].e;
        const double* gr = D->root_r;
        const double* ge = D->root_e;
        for (int i = threadIdx.x; i < N0; i += BT) {
            r[i] = gr[i];
            if (keep) e[i] = ge[i];
        }
    }
    __syncthreads();
    SolveCtx c = sol_ctx(LD, &lds, red, blkpart, dyn_raw, dbg);
    if (dbg && threadIdx.x == 0) {
        dbg[4] = dbg[5] = dbg[6] = dbg[7] = 0;
        dbg[9] = dbg[10] = dbg[11] = dbg[12] = dbg[13] = 0;
        dbg[2] = wall_clock64();
        dbg[8] = clock64();
    }
    sol_cycle(c, k0, keep != 0);
    __syncthreads();
    if (dbg && threadIdx.x == 0) {
        dbg[3] = wall_clock64();
        dbg[8] = clock64() - dbg[8];
    }
    const double* res = sol_e(c, k0);
    double* ge = D->root_e;
    for (int i = threadIdx.x; i < N0; i += BT) ge[i] = res[i];
}

// (ipd_cycle_state.h)
void optin_small_kernels(ipd_ctx* ctx) {
    IPD_OPTIN_LDS(ctx, k_solve_small<true>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_solve_small<false>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_pcg_small<true>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_pcg_small<false>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_subcycle, IMAGE_LDS_OPTIN);
}

// the whole solve phase (cycles == 0) or `cycles` cycles without stopping rules as one single-workgroup launch
void launch_solve_small(ipd_ctx* ctx, CycleState* st, const double* b_dev, double* x, int cycles) {
    const CycleState::Image& im = st->img[IMG_SOLVE];
    if (st->solve_cached)
        hipLaunchKernelGGL(k_solve_small<true>, dim3(1), dim3(BT), im.lds, ctx->stream, (const SolveDesc*)im.desc,
                           b_dev, x, st->x2, st->hist, st->solve_out, cycles);
    else
        hipLaunchKernelGGL(k_solve_small<false>, dim3(1), dim3(BT), im.lds, ctx->stream, (const SolveDesc*)im.desc,
                           b_dev, x, st->x2, st->hist, st->solve_out, cycles);
    IPD_KERNEL_CHECK();
}

void launch_subcycle(ipd_ctx* ctx, CycleState* st, bool keep_e) {
    hipLaunchKernelGGL(k_subcycle, dim3(1), dim3(BT), st->img[IMG_SUB].lds, ctx->stream,
                       (const SolveDesc*)st->img[IMG_SUB].desc, keep_e ? 1 : 0);
    IPD_KERNEL_CHECK();
}

// ---- the whole AMG-PCG solve as one single-workgroup launch (ipd_amg_pcg_planned) ---------
bool amg_pcg_small_ok(ipd_amg* h) {
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    return st->small_ok && st->shard_ranks == 1;
}

void amg_pcg_small_launch(ipd_amg* h, const PcgSmallVecs& v, double tol, int maxit) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    IPD_REQUIRE(st && st->small_ok && st->shard_ranks == 1, IPD_E_ARG,
                "AMG-PCG: the hierarchy is not planned for the single-workgroup solve");
    IPD_REQUIRE(maxit >= 0 && maxit <= PCG_SMALL_MAXIT, IPD_E_ARG, "AMG-PCG: maxit beyond the one-launch cap");
    PcgSmallArgs a;
    a.e = v.e;
    a.d = v.d;
    a.r = v.r;
    a.p = v.p;
    a.q = v.q;
    a.w_old = v.w_old;
    a.tol2 = tol * tol;
    a.maxit = maxit;
    a.out = v.out;
    if (st->solve_cached)
        hipLaunchKernelGGL(k_pcg_small<true>, dim3(1), dim3(BT), st->img[IMG_SOLVE].lds, ctx->stream,
                           (const SolveDesc*)st->img[IMG_SOLVE].desc, a);
    else
        hipLaunchKernelGGL(k_pcg_small<false>, dim3(1), dim3(BT), st->img[IMG_SOLVE].lds, ctx->stream,
                           (const SolveDesc*)st->img[IMG_SOLVE].desc, a);
    IPD_KERNEL_CHECK();
}
