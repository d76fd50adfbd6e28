// AMG-preconditioned conjugate gradients on a device hierarchy: the loop of PCG.m:68-87 with the
// preconditioner M(r) = one cycle of the hierarchy from a zero guess (MG_Vcycle(r,isnsp,1) or
// MG_Wcycle(r,isnsp,1) with the hierarchy's own cycle, smoth, isnsp, bigph and fnode) and the
// flexible (Polak-Ribiere) beta = (r'w - r'w_old) / delta_old.
//
// Why not PCG.m's Fletcher-Reeves beta = delta_new / delta_old: with isnsp = 1 the cycle is not a
// symmetric operator (the kernel-augmented pre-smoother P0 + R(I - A P0) is not the transpose of the
// post-smoother P0 + R'(I - A P0)), and the coarsest solve is a PCG to 1e-11, which is not linear at
// all.  For a symmetric linear M both forms agree in exact arithmetic.
//
// One iteration = K1 + K2 + the cycle + K3, and one host read (the scalar block, for the loop test):
//   K1 k_kry_dir_spmv  p_new = w + beta p_old formed inside the level-1 row walk's gather (p_old is
//                      only read, so no workgroup sees a neighbour's half-written p), p_new and
//                      w_old = w stored for the owned rows, q = A_1 p_new, partials of p_new'q; the
//                      last workgroup forms alpha.  With START it forms r = e - A_1 d0 instead.
//   K2 k_kry_update    d += alpha p ; r -= alpha q, the new r also written into the cycle's input
//                      L[1].r (the PCG keeps its own r: no cycle path is then trusted to leave
//                      L[1].r alone).
//   cycle              amg_apply_cycle: w = L[1].e.
//   K3 k_kry_dots      r'w and r'w_old in one pass; the last workgroup forms delta_new, beta,
//                      resk and the stop flag.
// Reductions are per-workgroup partials summed in fixed workgroup order by the workgroup that
// arrives last (agent-scope release / acquire around a ticket it resets itself): no float
// atomics, the same bits run to run.  Separate multiplies and adds (-ffp-contract=off).
//
// Always the launch-path cycle: the resident kernels (k_resident*, k_solve_small) run whole
// Class_AMG loops and are not used here.  ipd_amg_pcg_planned (below) is the form that runs the same
// loop as ONE single-workgroup launch (k_pcg_small, ipd_small.hip) on a hierarchy planned for the
// single-workgroup solve, and is this file's amg_pcg_dev on every other hierarchy.
#include "ipd_amg_internal.h"

#include <cmath>
#include <cstring>

#include "ipd_cycle_dev.h"
#include "ipd_cycle_phases.h"
#include "ipd_krylov.h"

struct KrylovState {
    int N = 0;
    int G1 = 0, G3 = 0;          // workgroups of K1 / of K2 and K3
    double* p[2] = {nullptr, nullptr};
    double* q = nullptr;
    double* w_old = nullptr;
    double* d = nullptr;
    double* r = nullptr;
    double* sc = nullptr;        // SC_N scalars
    double* part1 = nullptr;     // G1 partials of p'q
    double* part3 = nullptr;     // 2 x G3 partials of r'w, r'w_old
    unsigned* cnt = nullptr;     // tickets of K1 and K3
    double* out = nullptr;       // k_pcg_small's read-back: it, res, delta_0, -, resk[PCG_SMALL_MAXIT]
    int last_mode = -1;          // how the most recent AMG-PCG call ran (ipd_amg_pcg_mode)
};

struct KryDirArgs {
    LevelDev lv;
    const double* w;       // preconditioned residual; START: the initial guess (NULL: zero)
    const double* p_old;   // NULL: first direction (beta = 0, p_old not read)
    double* p_new;
    double* w_old;
    double* q;
    const double* e;       // START: right-hand side
    double* r;             // START: residual (the PCG's copy) ...
    double* r1;            // ... and the cycle's input L[1].r
    double* d;             // START: d = d0
    double* sc;
    double* part;
    unsigned* cnt;
};

// Level-1 row walk of phase_top (ipd_cycle_phases.h), gathering p_new = w + beta p_old.
template <bool STAGED, bool PAD, bool START>
__global__ __launch_bounds__(BT) void k_kry_dir_spmv(KryDirArgs a) {
    __shared__ PhaseLds lds;
    extern __shared__ __attribute__((aligned(16))) double xs[];
    const LevelDev& lv = a.lv;
    const int b = blockIdx.x, G = gridDim.x;
    const int tid = threadIdx.x;
    const int N = lv.N, L = lv.L, gpb = BT / L;
    const int g = tid / L, gl = tid - g * L;
    const bool uni = L >= 64;
    const int niter = (N + G * gpb - 1) / (G * gpb);
    const double* __restrict__ w = a.w;
    const double* __restrict__ po = a.p_old;
    const double beta = (!START && po) ? a.sc[SC_BETA] : 0.0;
    auto xglobal = [&](int j) -> double {
        if (START) return w ? w[j] : 0.0;
        return po ? w[j] + beta * po[j] : w[j];
    };
    auto xlds = [&](int j) { return xs[j]; };
    int row = uniform_if(b * gpb + g, uni);
    bool valid = row < N;
    bool owner = valid && gl == 0;
    RowCursor rc;
    RowBatch bt;
    row_open<PAD>(lv, row, valid, owner, gl, L, rc, bt);
    if (STAGED) {
        vec_pass(N, [&](int j) { return xglobal(j); }, [&](int j, double v) { xs[j] = v; });
        __syncthreads();
    }
    double acc = 0.0;
    for (int it = 0; it < niter; ++it) {
        if (it > 0) {
            row = uniform_if((it * G + b) * gpb + g, uni);
            valid = row < N;
            owner = valid && gl == 0;
            row_open<PAD>(lv, row, valid, owner, gl, L, rc, bt);
        }
        double s = STAGED ? row_finish<PAD>(lv, rc, bt, gl, L, xlds)
                          : row_finish<PAD>(lv, rc, bt, gl, L, xglobal);
        double dummy;
        s = reduce_rows(s, L, false, 0.0, &dummy, &lds);
        if (owner) {
            const double xo = STAGED ? xs[row] : xglobal(row);
            if (PAD) s += rc.dg * xo;
            if (START) {                                                          // PCG.m:68
                const double ri = a.e[row] - s;
                a.r[row] = ri;
                a.r1[row] = ri;
                a.d[row] = xo;
            } else {
                a.p_new[row] = xo;
                a.w_old[row] = w[row];
                a.q[row] = s;                                                     // :77
                acc += xo * s;
            }
        }
    }
    if (START) return;
    block_totals_to(acc, a.part + b, 0.0, nullptr, &lds);
    if (tid >= 64 || !kry_last_arrival(a.cnt)) return;
    const double pq = kry_sum_parts(a.part, G, 1);
    if (tid == 0) pcg_step_alpha(a.sc, pq);                                       // :77-78
}

// d += alpha p ; r -= alpha q (both copies of r)                                 PCG.m:79
__global__ __launch_bounds__(BT) void k_kry_update(int N, const double* __restrict__ sc,
                                                   const double* __restrict__ p,
                                                   const double* __restrict__ q, double* __restrict__ d,
                                                   double* __restrict__ r, double* __restrict__ r1) {
    const double alpha = sc[SC_ALPHA];
    for (int i = blockIdx.x * BT + threadIdx.x; i < N; i += gridDim.x * BT) {
        d[i] = d[i] + alpha * p[i];
        const double ri = r[i] - alpha * q[i];
        r[i] = ri;
        r1[i] = ri;
    }
}

struct KryDotArgs {
    int N;
    const double* r;
    const double* w;
    const double* w_old;   // FIRST: not read
    double tol2;           // retol^2
    double maxit;
    double* sc;
    double* part;          // [r'w | r'w_old] x G
    unsigned* cnt;
};

template <bool FIRST>
__global__ __launch_bounds__(BT) void k_kry_dots(KryDotArgs a) {
    __shared__ PhaseLds lds;
    const int G = gridDim.x, b = blockIdx.x, tid = threadIdx.x;
    double rw = 0.0, rwo = 0.0;
    for (int i = b * BT + tid; i < a.N; i += G * BT) {
        const double ri = a.r[i];
        rw += ri * a.w[i];
        if (!FIRST) rwo += ri * a.w_old[i];
    }
    block_totals_to(rw, a.part + 2 * b, rwo, FIRST ? nullptr : a.part + 2 * b + 1, &lds);
    if (tid >= 64 || !kry_last_arrival(a.cnt)) return;
    const double dn = kry_sum_parts(a.part, G, 2);
    const double s_wo = FIRST ? 0.0 : kry_sum_parts(a.part + 1, G, 2);
    if (tid == 0) pcg_step<FIRST>(a.sc, dn, s_wo, a.maxit, a.tol2);               // PCG.m:70-72, :81-85, :76
}

static KrylovState* krylov_state(ipd_amg* h, int N, int G1, int G3) {
    if (!h->kry) {
        auto ks = std::make_shared<KrylovState>();
        Arena& ar = *h->arena;   // the hierarchy's own storage (not the per-call zero pool)
        ks->N = N;
        ks->G1 = G1;
        ks->G3 = G3;
        for (auto& v : ks->p) v = ar.alloc<double>((size_t)N);
        ks->q = ar.alloc<double>((size_t)N);
        ks->w_old = ar.alloc<double>((size_t)N);
        ks->d = ar.alloc<double>((size_t)N);
        ks->r = ar.alloc<double>((size_t)N);
        ks->sc = ar.alloc<double>(SC_N);
        ks->part1 = ar.alloc<double>((size_t)G1);
        ks->part3 = ar.alloc<double>(2 * (size_t)G3);
        ks->cnt = ar.alloc<unsigned>(2);
        ks->out = ar.alloc<double>(4 + (size_t)PCG_SMALL_MAXIT);
        h->kry = ks;
    }
    IPD_REQUIRE(h->kry->N == N && h->kry->G1 == G1 && h->kry->G3 == G3, IPD_E_ARG,
                "AMG-PCG: level-1 geometry changed");
    return h->kry.get();
}

// What both routes start with: the cycle check, level 1's row walk, the hierarchy's one KrylovState
struct KrylovCall {
    LevelDev lv;
    int staged = 0, G1 = 1, G3 = 1, N = 0;
    KrylovState* ks = nullptr;
};
static KrylovCall krylov_call(ipd_amg* h, PcgRoute route) {
    const int cyc = h->opts.cycle;
    IPD_REQUIRE(cyc == 'v' || cyc == 'w', IPD_E_ARG,
                "AMG-PCG: the hierarchy's cycle must be 'v' or 'w' (any other value applies no correction)");
    KrylovCall c;
    IPD_REQUIRE(amg_level1_walk(h, &c.lv, &c.staged, &c.G1), IPD_E_UNSUPPORTED,
                "AMG-PCG: level 1 is sharded over ranks");
    c.N = c.lv.N;
    c.G3 = krylov_g3(c.N, h->ctx->num_cu);
    c.ks = krylov_state(h, c.N, c.G1, c.G3);
    c.ks->last_mode = route;
    return c;
}

// [d,it,res,resk] = AMG_PCG(h,e,pcg_options) on device vectors; resk: host, maxit slots or NULL
static void amg_pcg_dev(ipd_amg* h, const double* e, const double* guess, double tol, long long maxit,
                        double* d_out, long long* it_out, double* res_out, double* resk) {
    ipd_ctx* ctx = h->ctx;
    const KrylovCall kc = krylov_call(h, PCG_LAUNCHES);
    const LevelDev& lv = kc.lv;
    const int staged = kc.staged, G1 = kc.G1, G3 = kc.G3, N = kc.N;
    KrylovState* ks = kc.ks;
    const bool pad = lv.S > 0;
    const size_t dyn = staged ? sizeof(double) * (size_t)N : 0;
    double* r1 = h->L[1].r;
    // tickets start at zero on every call (the last arriver resets its own, this covers a launch
    // that never completed)
    IPD_HIP(hipMemsetAsync(ks->cnt, 0, 2 * sizeof(unsigned), ctx->stream));

    KryDirArgs ka{};
    ka.lv = lv;
    ka.w = guess;                                                                 // PCG.m:68
    ka.e = e;
    ka.r = ks->r;
    ka.r1 = r1;
    ka.d = ks->d;
    dispatch_staged_pad(staged, pad, [&](auto S, auto P) {
        hipLaunchKernelGGL((k_kry_dir_spmv<decltype(S)::value, decltype(P)::value, true>), dim3(G1), dim3(BT),
                           decltype(S)::value ? dyn : 0, ctx->stream, ka);
    });
    IPD_KERNEL_CHECK();
    KryDotArgs kd{};
    kd.N = N;
    kd.r = ks->r;
    kd.w_old = ks->w_old;
    kd.tol2 = tol * tol;
    kd.maxit = (double)maxit;
    kd.sc = ks->sc;
    kd.part = ks->part3;
    kd.cnt = ks->cnt + 1;
    amg_apply_cycle(h);                                                           // :69
    kd.w = h->L[1].e;
    hipLaunchKernelGGL(k_kry_dots<true>, dim3(G3), dim3(BT), 0, ctx->stream, kd);
    IPD_KERNEL_CHECK();
    double sc[SC_N];
    ctx->fetch(ks->sc, sc, SC_N);

    ka = KryDirArgs{};
    ka.lv = lv;
    ka.w_old = ks->w_old;
    ka.q = ks->q;
    ka.sc = ks->sc;
    ka.part = ks->part1;
    ka.cnt = ks->cnt;
    int cur = 0;   // p[cur]: the current direction
    bool have_p = false;
    long long it = 0;
    while (sc[SC_STOP] == 0.0) {                                                  // :76
        ka.w = h->L[1].e;
        ka.p_old = have_p ? ks->p[cur] : nullptr;
        ka.p_new = ks->p[cur ^ 1];
        dispatch_staged_pad(staged, pad, [&](auto S, auto P) {
            hipLaunchKernelGGL((k_kry_dir_spmv<decltype(S)::value, decltype(P)::value, false>), dim3(G1), dim3(BT),
                               decltype(S)::value ? dyn : 0, ctx->stream, ka);
        });
        IPD_KERNEL_CHECK();                                        // :77-78, :83
        cur ^= 1;
        have_p = true;
        hipLaunchKernelGGL(k_kry_update, dim3(G3), dim3(BT), 0, ctx->stream, N, (const double*)ks->sc,
                           (const double*)ks->p[cur], (const double*)ks->q, ks->d, ks->r, r1);
        IPD_KERNEL_CHECK();                                                       // :79
        amg_apply_cycle(h);                                                       // :80
        kd.w = h->L[1].e;
        hipLaunchKernelGGL(k_kry_dots<false>, dim3(G3), dim3(BT), 0, ctx->stream, kd);
        IPD_KERNEL_CHECK();                                                       // :81-82, :84-85
        ctx->fetch(ks->sc, sc, SC_N);
        it = (long long)sc[SC_IT];
        if (resk) resk[pcg_resk_slot(0, maxit, it)] = sc[SC_RES];
    }
    IPD_HIP(hipMemcpyAsync(d_out, ks->d, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
    if (it_out) *it_out = it;
    if (res_out) *res_out = sc[SC_RES];                                           // :88
    ctx->sync();
}

// amg_pcg_dev's contract; on a hierarchy planned for the single-workgroup solve the whole loop is one
// launch of k_pcg_small and one read-back, on every other hierarchy (and for maxit beyond
// PCG_SMALL_MAXIT) it IS amg_pcg_dev.
void amg_pcg_planned_dev(ipd_amg* h, const double* e, const double* guess, double tol, long long maxit,
                         double* d_out, long long* it_out, double* res_out, double* resk) {
    if (pcg_route(amg_pcg_small_ok(h), maxit) == PCG_LAUNCHES) {
        amg_pcg_dev(h, e, guess, tol, maxit, d_out, it_out, res_out, resk);
        return;
    }
    ipd_ctx* ctx = h->ctx;
    const KrylovCall kc = krylov_call(h, PCG_ONE_LAUNCH);   // the launch path's vectors: one state per hierarchy
    const int N = kc.N;
    KrylovState* ks = kc.ks;
    if (guess)
        IPD_HIP(hipMemcpyAsync(ks->d, guess, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
    else
        IPD_HIP(hipMemsetAsync(ks->d, 0, sizeof(double) * (size_t)N, ctx->stream));
    PcgSmallVecs v;
    v.e = e;
    v.d = ks->d;
    v.r = ks->r;
    v.p = ks->p[0];
    v.q = ks->q;
    v.w_old = ks->w_old;
    v.out = ks->out;
    amg_pcg_small_launch(h, v, tol, (int)maxit);
    std::vector<double> out(4 + (size_t)maxit);
    ctx->fetch(ks->out, out.data(), out.size());
    const long long it = (long long)out[0];
    if (resk && it > 0) std::memcpy(resk, out.data() + 4, sizeof(double) * (size_t)it);
    IPD_HIP(hipMemcpyAsync(d_out, ks->d, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
    if (it_out) *it_out = it;
    if (res_out) *res_out = out[1];
    ctx->sync();
}

extern "C" int ipd_amg_pcg_mode(const ipd_amg* h, int32_t* mode) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && mode, IPD_E_ARG, "NULL argument");
        *mode = h->kry ? h->kry->last_mode : -1;
    });
}

typedef void (*PcgDevFn)(ipd_amg*, const double*, const double*, double, long long, double*, long long*, double*,
                         double*);

// a single-vector entry around `solve` (amg_pcg_dev or amg_pcg_planned_dev): device vectors as they are, host
// vectors through the call's scratch
static int pcg_entry(PcgDevFn solve, bool host, ipd_amg* h, const double* e, const double* guess,
                     const ipd_pcg_opts* o, double* d, int64_t* it, double* res, double* resk) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && e && d, IPD_E_ARG, "NULL argument");
        double tol;
        long long maxit;
        pcg_opts_of(o, &tol, &maxit);
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        const size_t N = (size_t)h->L[1].A.nr;
        const double *de = e, *dg = guess;
        double* dd = d;
        if (host) {
            double* up = ctx->scratch->alloc<double>(N);
            dd = ctx->scratch->alloc<double>(N);
            ctx->upload(up, e, N);
            de = up;
            if (guess) {
                up = ctx->scratch->alloc<double>(N);
                ctx->upload(up, guess, N);
                dg = up;
            }
        }
        long long its = 0;
        solve(h, de, dg, tol, maxit, dd, &its, res, resk);
        if (it) *it = its;
        if (host) ctx->fetch(dd, d, N);
    });
}

extern "C" int ipd_amg_pcg_planned_dev(ipd_amg* h, const double* e_dev, const double* guess_dev,
                                       const ipd_pcg_opts* o, double* d_dev, int64_t* it, double* res,
                                       double* resk) {
    return pcg_entry(amg_pcg_planned_dev, false, h, e_dev, guess_dev, o, d_dev, it, res, resk);
}

extern "C" int ipd_amg_pcg_planned(ipd_amg* h, const double* e, const double* guess, const ipd_pcg_opts* o,
                                   double* d, int64_t* it, double* res, double* resk) {
    return pcg_entry(amg_pcg_planned_dev, true, h, e, guess, o, d, it, res, resk);
}

extern "C" int ipd_amg_pcg_dev(ipd_amg* h, const double* e_dev, const double* guess_dev,
                               const ipd_pcg_opts* o, double* d_dev, int64_t* it, double* res,
                               double* resk) {
    return pcg_entry(amg_pcg_dev, false, h, e_dev, guess_dev, o, d_dev, it, res, resk);
}

extern "C" int ipd_amg_pcg(ipd_amg* h, const double* e, const double* guess, const ipd_pcg_opts* o,
                           double* d, int64_t* it, double* res, double* resk) {
    return pcg_entry(amg_pcg_dev, true, h, e, guess, o, d, it, res, resk);
}
