// Class 2's bordered Newton systems on the device: AMG4POT (Class2/AMG4POT.m:27-55, Sherman-Morrison around
// two Hybrid_AMG solves), PCG4POT (Class2/PCG4POT.m:27-39, the same around two aug_PCG solves) and the
// dense routes on the bordered Jacobian itself (APD_SsN_Class2.m:152-161).
#pragma clang fp contract(off)

#include <thread>

#include "ipd_hybrid_state.h"
#include "ipd_kkt.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// AMG4POT                                              (Class2/AMG4POT.m:27-55)
// ---------------------------------------------------------------------------
__global__ void k_mask_mul(size_t len, const uint8_t* __restrict__ s,
                           const double* __restrict__ phi, double* __restrict__ out,
                           double* __restrict__ part) {
    // out = s.*phi ; part[block] = sum phi.*(s.*phi)
    __shared__ double red[4];
    double acc = 0.0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < len; i += (size_t)gridDim.x * 256) {
        const double v = s[i] ? phi[i] : 0.0;
        out[i] = v;
        acc += phi[i] * v;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void k_axpby(int n, double a, const double* __restrict__ x, double b,
                        const double* __restrict__ y, double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = a * x[i] + b * y[i];
}

// sphi = s.*phi out of ctx->scratch; returns phi'*(s.*phi)
static double mask_mul(ipd_ctx* ctx, size_t mn, const uint8_t* s, const double* phi, double** sphi) {
    Arena& tmp = *ctx->scratch;
    *sphi = tmp.alloc<double>(mn);
    const int nb = (int)std::max<size_t>(1, std::min<size_t>((mn + 255) / 256, 1024));
    double* part = tmp.alloc<double>((size_t)nb);
    hipLaunchKernelGGL(k_mask_mul, dim3(nb), dim3(256), 0, ctx->stream, mn, s, phi, *sphi, part);
    IPD_KERNEL_CHECK();
    return host_sum(ctx, part, nb);
}

template <class SOLVE>
static void pot_reduce(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi,
                       double* zeta, HybridOut* out, SOLVE solve) {
    const int m = sys.m, n = sys.n, M = sys.M();
    Arena& tmp = *ctx->scratch;
    const double epss = sys.bk1, sg = 1.0 / sys.tk;                       // :31
    double* sphi = nullptr;
    const double phi_e = pot_phi_e(epss, sg, mask_mul(ctx, (size_t)m * n, s, phi, &sphi));   // :33
    double* v = tmp.alloc<double>((size_t)M);
    kkt_ax(ctx, sphi, sys.p, sys.q, m, n, v);                             // :34 v = Ax(s.*phi)
    const double z2 = ctx->fetch1(z + M);
    double* w = tmp.alloc<double>((size_t)M);
    hipLaunchKernelGGL(k_axpby, dim3(elems_grid(M)), dim3(256), 0, ctx->stream, M, 1.0, z,
                       pot_w_coeff(sg, phi_e, z2), (const double*)v, w);  // w = z1 - sg/phi_e*z2*v
    IPD_KERNEL_CHECK();
    double* vv = tmp.alloc<double>((size_t)M);
    double* ww = tmp.alloc<double>((size_t)M);
    HybridOut o1, o2;
    solve(v, vv, &o1);                                                    // :46
    solve(w, ww, &o2);                                                    // :47
    const double vvv = host_dot(ctx, v, vv, M);
    const double vww = host_dot(ctx, v, ww, M);
    const double tt = pot_tt(sg, phi_e, vvv);                             // :53
    hipLaunchKernelGGL(k_axpby, dim3(elems_grid(M)), dim3(256), 0, ctx->stream, M, 1.0,
                       (const double*)ww, tt * vww, (const double*)vv, zeta);  // zeta1
    IPD_KERNEL_CHECK();
    const double vz1 = host_dot(ctx, v, zeta, M);
    const double zeta2 = pot_zeta2(z2, sg, vz1, phi_e);                   // :54
    ctx->upload(zeta + M, &zeta2, 1);
    out->itamg = std::max(o1.itamg, o2.itamg);                            // :55
    out->resamg = std::max(o1.resamg, o2.resamg);
    out->num_comp = std::max(o1.num_comp, o2.num_comp);
    out->it_num = std::max(o1.it_num, o2.it_num);
}

// Row f3: AMG4POT solves two systems with the same Ae (Class2/AMG4POT.m:46-47) and the reference
// sets the hierarchy up twice.  The second setup draws fresh random numbers in mis_set, so only the
// rand-independent part (Ae, the components, levels 1-2) is shared: bit-identical to two full setups.
// (One hierarchy for both right-hand sides was measured in round 2 -- it changes zeta by 6.5e-9 and is
// slower, because the two solves no longer overlap -- and removed in round 4.)
void amg4pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi,
                 const AmgOpts& opts, ipd_rng* rng, double* zeta, HybridOut* out, StepDonors* step) {
    const bool no_donor = switch_on("IPD_NO_DONOR");
    if (switch_on("IPD_NO_POT_CONCURRENT")) {
        if (step) step->prev.clear();
        auto solve = [&](const double* rhs, double* x, HybridOut* o) {
            HybridCall plain(sharing_rule(CALL_PLAIN, false, false, no_donor));
            hybrid_amg(ctx, sys, rhs, opts, rng, x, o, plain, nullptr);
        };
        pot_reduce(ctx, sys, z, s, phi, zeta, out, solve);
        ctx->sync();
        return;
    }
    // The two systems Ae*vv = v and Ae*ww = w are independent (Class2/AMG4POT.m:46-47).  Their
    // guesses and hierarchies are drawn/built one after the other -- the rand stream is consumed
    // in the reference's order -- and their solve phases then run at the same time on two
    // streams: each is a chain of latency-bound launches that leaves the device mostly idle.
    ipd_ctx* aux = ipd_ctx_aux(ctx);
    AmgOpts popts = opts;
    popts.concurrent_pair = true;
    Deferred first, second;
    const bool same = step && step->same;   // the previous Newton step had this very system
    SystemCache system;
    HybridCall call1(sharing_rule(CALL_POT_FIRST, step != nullptr, same, no_donor));
    HybridCall call2(sharing_rule(CALL_POT_SECOND, step != nullptr, same, no_donor));
    call1.system = call2.system = &system;
    if (step) {
        call1.donors = &step->prev;
        call1.shared = &step->shared;
    }
    call2.donors = &call1.recorded;   // the second setup shares the first one's levels
    const bool keep = step && call1.rule.record;   // the first solve's hierarchies, for the next Newton step
    if (step && !keep) step->prev.clear();
    bool have_first = false;
    auto solve = [&](const double* rhs, double* x, HybridOut* o) {
        if (!have_first) {
            hybrid_amg(ctx, sys, rhs, popts, rng, x, o, call1, &first);
            have_first = true;
            return;
        }
        ctx->sync();   // rhs, H0, ... were produced on ctx's stream
        // (Letting the second setup overlap with the first solve phase as well was measured: no
        // gain -- the setup is bound by its host round trips -- so both setups stay on this
        // thread and only the solve phases, which consume no random numbers, run concurrently.)
        CallScope aux_scope(aux);
        // an injected component order (ipd_ctx_set_component_order) holds for both solves: without the
        // shared component cache (IPD_NO_DONOR=1) the second call finds the components itself
        aux->comp_order = ctx->comp_order;
        hybrid_amg(aux, sys, rhs, popts, rng, x, o, call2, &second);
        std::exception_ptr err;
        std::thread other([&] {
            try {
                aux->set_device();
                for (auto& fn : second) fn();
                aux->sync();
            } catch (...) {
                err = std::current_exception();
            }
        });
        std::exception_ptr err0;
        try {
            for (auto& fn : first) fn();
            ctx->sync();
        } catch (...) {
            err0 = std::current_exception();
        }
        other.join();
        first.clear();    // releases the hierarchies
        second.clear();
        if (keep)
            step->prev = std::move(call1.recorded);
        else
            call1.recorded.clear();
        if (err0) std::rethrow_exception(err0);
        if (err) std::rethrow_exception(err);
    };
    pot_reduce(ctx, sys, z, s, phi, zeta, out, solve);
}

// PCG4POT (Class2/PCG4POT.m:27-39) = amg4pot_dev's reduction with aug_PCG as the inner solve
void pcg4pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi, double tol,
                 long long maxit, double* zeta, HybridOut* out) {
    auto solve = [&](const double* rhs, double* x, HybridOut* o) { aug_pcg_dev(ctx, sys, rhs, tol, maxit, x, o); };
    pot_reduce(ctx, sys, z, s, phi, zeta, out, solve);
}

// ---------------------------------------------------------------------------
// Class 2, inner_solver = 1 and 2: the bordered Jacobian itself      (APD_SsN_Class2.m:152-161)
//   J = bk1*speye(M+1) + (cT + cH0)/tk,  cT = [T 0; 0 0],  cH0 = [H0 ss; ss' phi'*(s.*phi)],
//   ss = Ax(s.*phi)
// assembled densely ((M+1)^2 doubles: cold paths, bounded by the 2 GiB scratch limit)
// ---------------------------------------------------------------------------
__global__ void k_border(int M, int ld, const double* __restrict__ ss, double itk /* tk */, double corner,
                         double* __restrict__ D) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= M; i += gridDim.x * blockDim.x) {
        if (i < M) {
            const double v = ss[i] / itk;            // (0 + ss)/tk
            D[(size_t)i * ld + M] = v;
            D[(size_t)M * ld + i] = v;
        } else {
            D[(size_t)M * ld + M] = corner;
        }
    }
}

static double* pot_jacobian_dense(ipd_ctx* ctx, const NewtonSys& sys, const uint8_t* s, const double* phi) {
    const int m = sys.m, n = sys.n, M = sys.M(), N = M + 1;
    const double bk1 = sys.bk1, tk = sys.tk;
    Arena& tmp = *ctx->scratch;
    IPD_REQUIRE((size_t)N * N * 8 <= (size_t(2) << 30), IPD_E_LIMIT,
                "inner_solver 1/2 (class 2): dense Jacobian above 2 GiB");
    double* sphi = nullptr;
    const double pssp = mask_mul(ctx, (size_t)m * n, s, phi, &sphi);      // phi'*(s.*phi)
    double* ss = tmp.alloc<double>((size_t)M);
    kkt_ax(ctx, sphi, sys.p, sys.q, m, n, ss);                            // ss = Ax(s.*phi)
    Csr Jk;
    build_jk(ctx, tmp, sys, &Jk);                                         // bk1*I + (T + H0)/tk
    double* D = tmp.alloc<double>((size_t)N * N);
    IPD_HIP(hipMemsetAsync(D, 0, sizeof(double) * (size_t)N * N, ctx->stream));
    csr_expand_dense(ctx, Jk, D, N);
    hipLaunchKernelGGL(k_border, dim3(elems_grid(N)), dim3(256), 0, ctx->stream, M, N, (const double*)ss,
                       tk, bk1 + pssp / tk, D);
    IPD_KERNEL_CHECK();
    return D;
}

// zeta = J \ z                                                      (APD_SsN_Class2.m:155)
void direct_pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi,
                    double* zeta) {
    const int N = sys.M() + 1;
    double* D = pot_jacobian_dense(ctx, sys, s, phi);
    dense_chol_factor(ctx, D, N, N);
    if (zeta != z)
        IPD_HIP(hipMemcpyAsync(zeta, z, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
    dense_chol_solve(ctx, D, N, N, zeta, 1, 1);
}

// [zeta,itpcg,respcg] = PCG(J,z,pcg_options)                         (APD_SsN_Class2.m:161)
void pcg_pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi, double tol,
                 long long maxit, double* zeta, HybridOut* out) {
    const int N = sys.M() + 1;
    Arena& tmp = *ctx->scratch;
    double* D = pot_jacobian_dense(ctx, sys, s, phi);
    Csr J;
    J.nr = J.nc = N;
    int* cnt = zeroed<int>(ctx, (size_t)N + 1);   // (biased counts: see ScanTail)
    J.rp = tmp.alloc<int>((size_t)N + 1);
    {
        TailTotal tt(ctx, cnt, J.rp, N);
        dense_rowcount(ctx, N, N, N, D, cnt, tt.t);
        int two[2] = {0, 0};
        tt.wait(two);
        J.nnz = two[0];
    }
    J.ci = tmp.alloc<int>((size_t)J.nnz);
    J.va = tmp.alloc<double>((size_t)J.nnz);
    dense_compact(ctx, N, N, N, D, J);
    long long it = 0;
    double res = 0.0;
    pcg_dev(ctx, J, z, nullptr, tol, maxit, 2, zeta, &it, &res, nullptr);
    out->itamg = (int)std::min<long long>(it, 2147483647LL);
    out->resamg = res;
    out->num_comp = 0;
    out->it_num = 0;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static int amg4pot_host(ipd_ctx* ctx, const ipd_prob* pd, const AmgOpts& ao, ipd_rng* rng,
                        double* zeta, int32_t* itamg, double* resamg, int64_t info[2]) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && zeta, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        CompOrderScope order_scope(ctx);
        const ProbDev d = upload_prob(ctx, pd, true);
        HybridOut ho;
        amg4pot_dev(ctx, d.sys, d.z, d.s, d.phi, ao, rng, d.zeta, &ho);
        ctx->fetch(d.zeta, zeta, d.len);
        report(ho, itamg, resamg, info);
    });
}

extern "C" int ipd_amg4pot(ipd_ctx* ctx, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                           double* zeta, int32_t* itamg, double* resamg, int64_t info[2]) {
    return amg4pot_host(ctx, pd, amg_fill_defaults(o), rng, zeta, itamg, resamg, info);
}
// AMG4POT(prob_data, amg_options, 'amg_pcg'): both Hybrid_AMG calls with AMG-PCG as the inner solver
extern "C" int ipd_amg4pot_pcg(ipd_ctx* ctx, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                               double* zeta, int32_t* itamg, double* resamg, int64_t info[2]) {
    return amg4pot_host(ctx, pd, amg_fill_krylov(o), rng, zeta, itamg, resamg, info);
}
// AMG4POT(prob_data, amg_options, 'twogrid')                      Class2/AMG4POT.m:48-51
extern "C" int ipd_amg4pot_twogrid(ipd_ctx* ctx, const ipd_prob* pd, const ipd_amg_opts* o,
                                   ipd_rng* rng, double* zeta, int32_t* itamg, double* resamg,
                                   int64_t info[2]) {
    return amg4pot_host(ctx, pd, amg_fill_twogrid_defaults(o), rng, zeta, itamg, resamg, info);
}
