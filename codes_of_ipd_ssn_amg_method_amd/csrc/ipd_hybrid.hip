// Hybrid_AMG on the device                                           (Hybrid_AMG.m:12-113)
//
// Rescaling and assembly are ipd_newton_sys.hip's, the components ipd_components.hip's; every routing
// decision is plan_route's (ipd_hybrid_plan.h).  What is left here executes a HybridRoute: one
// Class_AMG setup and solve per large component, one launch for the small ones.
#pragma clang fp contract(off)

#include <atomic>
#include <cstdio>
#include <string>

#include "ipd_hybrid_state.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// small components: u(pk) = Ae(pk,pk) \ f(pk)              (Hybrid_AMG.m:85-91)
// ---------------------------------------------------------------------------
// The system is block diagonal with SPD blocks of at most HYBRID_N0 rows: one
// workgroup per block factors its dense copy in LDS (Cholesky) and solves.
__global__ __launch_bounds__(256) void k_small_blocks(const int* __restrict__ boff,
                                                      const int* __restrict__ nodes,
                                                      const int* __restrict__ local,
                                                      const int* __restrict__ rp,
                                                      const int* __restrict__ ci,
                                                      const double* __restrict__ va,
                                                      const double* __restrict__ f,
                                                      double* __restrict__ u,
                                                      int* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int blk = blockIdx.x;
    const int o = boff[blk], nb = boff[blk + 1] - o;
    const int ld = nb + 1;
    double* A = reinterpret_cast<double*>(smem_raw);  // nb x ld, row-major
    double* y = A + (size_t)nb * ld;
    const int tid = threadIdx.x;
    for (int k = tid; k < nb * ld; k += 256) A[k] = 0.0;
    __syncthreads();
    for (int li = tid; li < nb; li += 256) {
        const int i = nodes[o + li];
        for (int t = rp[i]; t < rp[i + 1]; ++t) A[li * ld + local[ci[t]]] = va[t];
        y[li] = f[i];
    }
    __syncthreads();
    // right-looking Cholesky, lower triangle
    for (int k = 0; k < nb; ++k) {
        const double akk = A[k * ld + k];
        if (!(akk > 0.0)) {
            if (tid == 0) *bad = 1;
            return;  // uniform: every thread reads the same akk
        }
        const double lkk = sqrt(akk);
        __syncthreads();
        for (int i = k + tid; i < nb; i += 256) A[i * ld + k] = (i == k) ? lkk : A[i * ld + k] / lkk;
        __syncthreads();
        const int rem = nb - k - 1;
        for (int idx = tid; idx < rem * rem; idx += 256) {
            const int i = k + 1 + idx / rem, j = k + 1 + idx % rem;
            if (j <= i) A[i * ld + j] -= A[i * ld + k] * A[j * ld + k];
        }
        __syncthreads();
    }
    // forward and backward substitution by thread 0 of each wave-0 lane set (nb <= HYBRID_N0)
    if (tid == 0) {
        for (int i = 0; i < nb; ++i) {
            double s = y[i];
            for (int j = 0; j < i; ++j) s -= A[i * ld + j] * y[j];
            y[i] = s / A[i * ld + i];
        }
        for (int i = nb - 1; i >= 0; --i) {
            double s = y[i];
            for (int j = i + 1; j < nb; ++j) s -= A[j * ld + i] * y[j];
            y[i] = s / A[i * ld + i];
        }
    }
    __syncthreads();
    for (int li = tid; li < nb; li += 256) u[nodes[o + li]] = y[li];
}

static void small_blocks(ipd_ctx* ctx, const HybridRoute& rt, const Csr& Ae, const double* f, double* u) {
    ProfScope ps(ctx, PROF_SMALL_BLOCKS);
    Arena& tmp = *ctx->scratch;
    int* d_boff = tmp.alloc<int>(rt.boff.size());
    int* d_nodes = tmp.alloc<int>(rt.nodes.size());
    int* d_local = tmp.alloc<int>(rt.local.size());
    int* bad = tmp.alloc<int>(1);
    ctx->upload(d_boff, rt.boff.data(), rt.boff.size());
    ctx->upload(d_nodes, rt.nodes.data(), rt.nodes.size());
    ctx->upload(d_local, rt.local.data(), rt.local.size());
    IPD_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    IPD_OPTIN_LDS(ctx, k_small_blocks, HYBRID_SMALL_LDS_OPTIN);
    hipLaunchKernelGGL(k_small_blocks, dim3((unsigned)rt.boff.size() - 1), dim3(256), rt.small_lds, ctx->stream,
                       d_boff, d_nodes, d_local, Ae.rp, Ae.ci, Ae.va, f, u, bad);
    IPD_KERNEL_CHECK();
    IPD_REQUIRE(ctx->fetch1(bad) == 0, IPD_E_NUMERIC,
                "Hybrid_AMG: a small diagonal block is not positive definite");
}

// ---------------------------------------------------------------------------
// one Class_AMG solve
// ---------------------------------------------------------------------------
struct MaskHint {   // p, q, tk of the rescaled system when A is the whole Ae (else p == NULL)
    const double* p = nullptr;
    const double* q = nullptr;
    int m = 0, n = 0;
    double tk = 0.0;
};

// Guess + setup now (consumes rand); returns the solve phase, which fills *it / *rel_res.
// Row f3: which setups are offered whose hierarchy, and which are kept, is call.rule (sharing_rule,
// ipd_hybrid_plan.h).  A setup that takes a donor shares only the rand-independent part (levels 1-2):
// bit-identical to a full setup.
static std::function<void(int*, double*)> class_amg_prepare(
    ipd_ctx* ctx, const Csr& A, const double* f, AmgOpts o, int isnsp, long long fnode, double gscale,
    ipd_rng* rng, double* u_out, const MaskHint& mh, HybridCall& call) {
    const int N = A.nr;
    o.isnsp = isnsp;
    o.fnode = fnode;
    std::vector<double> g((size_t)N);
    rng->fill(g.data(), N);                       // Hybrid_AMG.m:40 / :69  bk1*tk*rand(size(f))
    for (double& v : g) v = gscale * v;
    double* dg = ctx->scratch->alloc<double>((size_t)N);
    ctx->upload(dg, g.data(), (size_t)N);
    std::shared_ptr<ipd_amg> own;
    {
        ProfScope ps(ctx, PROF_AMG_SETUP);
        std::shared_ptr<ipd_amg> donor;
        if (call.rule.from != DONORS_NONE && call.next_donor < call.donors->size())
            donor = (*call.donors)[call.next_donor++];
        own = std::shared_ptr<ipd_amg>(amg_setup(ctx, A, o, rng, donor), ipd_amg_destroy);
        // matrix-free level 1 where it pays (policy in amg_attach_maskop); not under AMG-PCG, whose
        // level-1 product walks A_1's rows and whose cycle is then the CSR one throughout
        if (mh.p && o.bigph && !o.krylov) amg_attach_maskop(own.get(), mh.p, mh.q, mh.m, mh.n, mh.tk, true);
        if (call.rule.record) call.recorded.push_back(own);
        if (call.rule.count && own->donor) ++*call.shared;
    }
    ipd_amg* h = own.get();
    const bool krylov = o.krylov;
    const double pcg_tol = o.retol;
    const long long pcg_maxit = o.maxit;
    return [ctx, h, own, f, dg, u_out, krylov, pcg_tol, pcg_maxit](int* it, double* rel_res) {
        int32_t its = 0;
        double rr = 0.0;
        {
            ProfScope ps(ctx, PROF_AMG_SOLVE);
            if (krylov) {   // every piece of PCG state belongs to h: right for either of AMG4POT's two threads
                long long itp = 0;
                amg_pcg_planned_dev(h, f, dg, pcg_tol, pcg_maxit, u_out, &itp, &rr, nullptr);
                its = (int32_t)itp;
            } else {
                amg_solve_dev(h, f, dg, u_out, &its, &rr, nullptr, nullptr);
            }
        }
        *it = its;
        *rel_res = rr;
    };
}

// Debugging aid: IPD_DUMP_SYSTEM=<prefix> IPD_DUMP_CALLS=<lo>-<hi> writes the rescaled Newton
// systems Ae*u = f of those Hybrid_AMG calls (counted per process from 0) to
// <prefix><call>.bin: int64 M, nf, nnz; int32 rp[M+1], ci[nnz]; double va[nnz], f[M].
// tests/read_system_dump.py reads them back, so a system a driver run produced can be put
// through the oracle.
static void dump_system(ipd_ctx* ctx, const Csr& Ae, const double* f, int nf) {
    static std::atomic<int> calls{0};
    const int call = calls++;
    const char* prefix = switch_value("IPD_DUMP_SYSTEM");
    if (!prefix) return;
    int lo = 0, hi = 0;
    if (const char* e = switch_value("IPD_DUMP_CALLS")) {
        if (sscanf(e, "%d-%d", &lo, &hi) < 2) hi = lo;
    }
    if (call < lo || call > hi) return;
    std::vector<int> rp((size_t)Ae.nr + 1), ci((size_t)Ae.nnz);
    std::vector<double> va((size_t)Ae.nnz), hf((size_t)Ae.nr);
    ctx->fetch(Ae.rp, rp.data(), rp.size());
    if (Ae.nnz) {
        ctx->fetch(Ae.ci, ci.data(), ci.size());
        ctx->fetch(Ae.va, va.data(), va.size());
    }
    ctx->fetch(f, hf.data(), hf.size());
    const std::string path = std::string(prefix) + std::to_string(call) + ".bin";
    FILE* fp = fopen(path.c_str(), "wb");
    IPD_REQUIRE(fp, IPD_E_ARG, "IPD_DUMP_SYSTEM: cannot open the output file");
    const int64_t head[3] = {Ae.nr, nf, Ae.nnz};
    fwrite(head, sizeof(int64_t), 3, fp);
    fwrite(rp.data(), sizeof(int), rp.size(), fp);
    fwrite(ci.data(), sizeof(int), ci.size(), fp);
    fwrite(va.data(), sizeof(double), va.size(), fp);
    fwrite(hf.data(), sizeof(double), hf.size(), fp);
    fclose(fp);
}

// ---------------------------------------------------------------------------
// Hybrid_AMG
// ---------------------------------------------------------------------------
void hybrid_amg(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const AmgOpts& opts, ipd_rng* rng, double* zeta,
                HybridOut* out, HybridCall& call, Deferred* later) {
    IPD_REQUIRE(rng, IPD_E_ARG, "Hybrid_AMG needs a rand stream");
    auto defer = [&](std::function<void()> fn) {   // run now, or in the caller's solve phase
        if (later)
            later->push_back(std::move(fn));
        else
            fn();
    };
    IPD_REQUIRE(sys.tk != 0.0, IPD_E_ARG, "tk must be nonzero");
    const int M = sys.M();
    Arena& tmp = *ctx->scratch;
    SystemCache own_system;
    SystemCache& system = call.rule.system ? *call.system : own_system;
    const bool reuse = system.valid;
    if (!reuse) {
        ProfScope ps(ctx, PROF_BUILD_AE);
        build_Ae(ctx, tmp, sys, &system.Ae);                              // :17-24
    }
    const Csr& Ae = system.Ae;
    double* f = tmp.alloc<double>((size_t)M);
    double* u = tmp.alloc<double>((size_t)M);
    double* dK = tmp.alloc<double>((size_t)M);
    scale_qp(ctx, sys, z, f);                                             // :24 f = Q0*z
    diag_k(ctx, sys, dK);
    IPD_HIP(hipMemsetAsync(u, 0, sizeof(double) * (size_t)M, ctx->stream));
    dump_system(ctx, Ae, f, sys.n);
    // components of A0 = Q0*H0*Q0: same pattern as H0 (qp has no zeros)     :27
    if (!reuse) {
        ProfScope ps(ctx, PROF_COMPONENTS);
        find_components(ctx, sys.H0, &system.cc);
        system.valid = true;
    }
    const Components& cc = system.cc;
    const HybridRoute rt = plan_route(cc, sys.n, opts.bigph != 0);
    IPD_REQUIRE(rt.one_sided < 0, IPD_E_NUMERIC, "Hybrid_AMG: a large component lies on one side of the bigraph");
    out->num_comp = cc.ncomp;
    out->itamg = 0;
    out->resamg = 0.0;
    out->it_num = rt.it_num;
    std::vector<double> hdK;
    if (sys.tdiag) {
        hdK.resize((size_t)M);
        ctx->fetch(dK, hdK.data(), (size_t)M);
    }
    const double* host_dk = sys.tdiag ? hdK.data() : nullptr;   // (no T: dK is zero)
    const double gscale = sys.bk1 * sys.tk;
    if (rt.connected) {                                                   // :30-48
        const LargeComponent& c = rt.large.front();
        const int isnsp = isnsp_of_dk(host_dk, cc.p.data(), c.len);
        MaskHint mh;
        mh.p = sys.p;
        mh.q = sys.q;
        mh.m = sys.m;
        mh.n = sys.n;
        mh.tk = sys.tk;
        auto run = class_amg_prepare(ctx, Ae, f, opts, isnsp, c.fnode, gscale, rng, u, mh, call);
        defer([run, out] { run(&out->itamg, &out->resamg); });
    } else {                                                              // :50-107
        ComponentCutter cutter(ctx, Ae);
        // [q; p] in the order of the unknowns: a large component's own q (its F rows) and p (its C rows) are
        // gathered from it for the mask form of its level 1 (amg_attach_maskop: the sub-matrix Ae(pk, pk) of a
        // component has the same rank-one structure, with the component's entries of p and q)
        double* qp = nullptr;
        if (rt.gather_qp) {
            qp = tmp.alloc<double>((size_t)M);
            IPD_HIP(hipMemcpyAsync(qp, sys.q, sizeof(double) * (size_t)sys.n, hipMemcpyDeviceToDevice, ctx->stream));
            IPD_HIP(hipMemcpyAsync(qp + sys.n, sys.p, sizeof(double) * (size_t)sys.m, hipMemcpyDeviceToDevice, ctx->stream));
        }
        for (const LargeComponent& c : rt.large) {                        // :55
            const int nk = c.len;
            const int* pk = cc.p.data() + c.off;
            Csr Ak;
            const int* d_pk = cutter.cut(pk, nk, &Ak);
            double* fk = tmp.alloc<double>((size_t)nk);
            double* dk = tmp.alloc<double>((size_t)nk);   // per component: the scatter may run later
            gather_dev(ctx, nk, d_pk, f, fk);
            const int isnsp = isnsp_of_dk(host_dk, pk, nk);   // :60-66
            MaskHint mhk;
            if (c.mask) {
                double* qpk = tmp.alloc<double>((size_t)nk);
                gather_dev(ctx, nk, d_pk, qp, qpk);
                mhk.q = qpk;
                mhk.p = qpk + c.fnode;
                mhk.n = c.fnode;
                mhk.m = nk - c.fnode;
                mhk.tk = sys.tk;
            }
            auto run = class_amg_prepare(ctx, Ak, fk, opts, isnsp, c.fnode, gscale, rng, dk, mhk, call);
            defer([run, out, ctx, nk, d_pk, dk, u] {
                int it = 0;
                double rr = 0.0;
                run(&it, &rr);
                scatter_dev(ctx, nk, d_pk, dk, u);                        // :77 u(pk) = dk
                out->itamg = std::max(out->itamg, it);
                out->resamg = std::max(out->resamg, rr);
            });
        }
        if (!rt.nodes.empty()) small_blocks(ctx, rt, Ae, f, u);           // :85-91, all together
    }
    defer([ctx, sys, u, zeta] { scale_qp(ctx, sys, u, zeta); });          // :113 zeta = Q0*u
}

void hybrid_amg_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const AmgOpts& opts, ipd_rng* rng,
                    double* zeta, HybridOut* out, StepDonors* step) {
    HybridCall call(sharing_rule(CALL_PLAIN, step != nullptr, step && step->same, switch_on("IPD_NO_DONOR")));
    // consecutive Newton steps with the same system (Hybrid_AMG.m:40-41 sets up per call)
    std::vector<std::shared_ptr<ipd_amg>> prev;
    if (step) {
        if (call.rule.from == DONORS_PREV_STEP) prev = std::move(step->prev);
        step->prev.clear();
        call.shared = &step->shared;
    }
    call.donors = &prev;
    hybrid_amg(ctx, sys, z, opts, rng, zeta, out, call, nullptr);
    if (call.rule.record) step->prev = std::move(call.recorded);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static int hybrid_host(ipd_ctx* ctx, const ipd_prob* pd, const AmgOpts& ao, ipd_rng* rng,
                       double* zeta, int32_t* itamg, double* resamg, int64_t info[2]) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && zeta, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        CompOrderScope order_scope(ctx);
        const ProbDev d = upload_prob(ctx, pd, false);
        HybridOut ho;
        hybrid_amg_dev(ctx, d.sys, d.z, ao, rng, d.zeta, &ho);
        ctx->fetch(d.zeta, zeta, d.len);
        report(ho, itamg, resamg, info);
    });
}

extern "C" int ipd_hybrid_amg(ipd_ctx* ctx, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                              double* zeta, int32_t* itamg, double* resamg, int64_t info[2]) {
    return hybrid_host(ctx, pd, amg_fill_defaults(o), rng, zeta, itamg, resamg, info);
}
AmgOpts amg_fill_krylov(const ipd_amg_opts* o) {
    AmgOpts ao = amg_fill_defaults(o);
    ao.krylov = true;
    return ao;
}
// Hybrid_AMG.m with every Class_AMG call replaced by setup + AMG-PCG from the same random guess
extern "C" int ipd_hybrid_amg_pcg(ipd_ctx* ctx, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                                  double* zeta, int32_t* itamg, double* resamg, int64_t info[2]) {
    return hybrid_host(ctx, pd, amg_fill_krylov(o), rng, zeta, itamg, resamg, info);
}
extern "C" int ipd_hybrid_twogrid(ipd_ctx* ctx, const ipd_prob* pd, const ipd_amg_opts* o,
                                  ipd_rng* rng, double* zeta, int32_t* itamg, double* resamg,
                                  int64_t info[2]) {
    return hybrid_host(ctx, pd, amg_fill_twogrid_defaults(o), rng, zeta, itamg, resamg, info);
}

static int hybrid_dev_entry(ipd_ctx* ctx, const ipd_dmat* H0, const double* t_dev, const double* p_dev,
                            const double* q_dev, int64_t m, int64_t n, double bk1, double tk,
                            const double* z_dev, const ipd_amg_opts* o, bool krylov, ipd_rng* rng,
                            double* zeta_dev, int32_t* itamg, double* resamg, int64_t info[2]) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && H0 && p_dev && q_dev && z_dev && zeta_dev, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(m > 0 && n > 0, IPD_E_ARG, "bad m/n");
        CallScope scope(ctx);
        CompOrderScope order_scope(ctx);
        NewtonSys sys;
        sys.H0 = H0->m;
        sys.tdiag = t_dev;
        sys.p = p_dev;
        sys.q = q_dev;
        sys.m = (int)m;
        sys.n = (int)n;
        sys.bk1 = bk1;
        sys.tk = tk;
        HybridOut ho;
        hybrid_amg_dev(ctx, sys, z_dev, krylov ? amg_fill_krylov(o) : amg_fill_defaults(o), rng, zeta_dev, &ho);
        ctx->sync();
        report(ho, itamg, resamg, info);
    });
}
extern "C" int ipd_hybrid_amg_dev(ipd_ctx* ctx, const ipd_dmat* H0, const double* t_dev,
                                  const double* p_dev, const double* q_dev, int64_t m, int64_t n,
                                  double bk1, double tk, const double* z_dev,
                                  const ipd_amg_opts* o, ipd_rng* rng, double* zeta_dev,
                                  int32_t* itamg, double* resamg, int64_t info[2]) {
    return hybrid_dev_entry(ctx, H0, t_dev, p_dev, q_dev, m, n, bk1, tk, z_dev, o, false, rng, zeta_dev, itamg,
                            resamg, info);
}
extern "C" int ipd_hybrid_amg_pcg_dev(ipd_ctx* ctx, const ipd_dmat* H0, const double* t_dev,
                                      const double* p_dev, const double* q_dev, int64_t m, int64_t n,
                                      double bk1, double tk, const double* z_dev,
                                      const ipd_amg_opts* o, ipd_rng* rng, double* zeta_dev,
                                      int32_t* itamg, double* resamg, int64_t info[2]) {
    return hybrid_dev_entry(ctx, H0, t_dev, p_dev, q_dev, m, n, bk1, tk, z_dev, o, true, rng, zeta_dev, itamg,
                            resamg, info);
}
