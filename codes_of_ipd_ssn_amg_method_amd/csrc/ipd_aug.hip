// aug_PCG on the device: PCG on the kernel-augmented system                  (aug_PCG.m:11-36)
#pragma clang fp contract(off)

#include "ipd_hybrid_state.h"

#include <algorithm>

// augAe = [Y'QK Y  Y'QK ; QK Y  Ae] with Y the component indicators and QK = bk1*Q + K/tk
// diagonal, so the first nc rows are  [d_c , qk_i for the members i of c]  and row nc+i is
// [qk_i at column c(i) , row i of Ae shifted by nc]; columns come out sorted.
__global__ void k_aug_qk(int M, int n, const double* __restrict__ p, const double* __restrict__ q,
                         const double* __restrict__ t, double bk1, double itk,
                         double* __restrict__ qk) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const double qp = i < n ? q[i] : -p[i - n];
        const double kk = t ? (qp * t[i]) * qp : 0.0;          // K = Q0*T*Q0
        qk[i] = bk1 * (qp * qp) + itk * kk;                     // aug_PCG.m:27
    }
}
__global__ void k_aug_rowlen(int nc, int M, const int* __restrict__ cr, const int* __restrict__ rp,
                             int* __restrict__ len) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nc + M; r += gridDim.x * blockDim.x)
        len[r] = r < nc ? 1 + cr[r + 1] - cr[r] : 1 + rp[r - nc + 1] - rp[r - nc];
}
// one wave per row of the augmented matrix; also the right-hand side [Y'f ; f]
__global__ __launch_bounds__(256) void k_aug_fill(int nc, int M, const int* __restrict__ cr,
                                                  const int* __restrict__ cp,
                                                  const int* __restrict__ blocks,
                                                  const double* __restrict__ qk,
                                                  const double* __restrict__ f,
                                                  const int* __restrict__ rp,
                                                  const int* __restrict__ ci,
                                                  const double* __restrict__ va,
                                                  const int* __restrict__ orp, int* __restrict__ oci,
                                                  double* __restrict__ ova, double* __restrict__ of) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int r = wave; r < nc + M; r += nwaves) {
        const int ob = orp[r];
        if (r < nc) {
            const int b = cr[r], e = cr[r + 1];
            if (lane == 0) {   // sums in ascending member order, like the sparse products
                double d = 0.0, fs = 0.0;
                for (int t = b; t < e; ++t) {
                    d += qk[cp[t]];
                    fs += f[cp[t]];
                }
                oci[ob] = r;
                ova[ob] = d;
                of[r] = fs;
            }
            for (int t = b + lane; t < e; t += 64) {
                oci[ob + 1 + (t - b)] = nc + cp[t];
                ova[ob + 1 + (t - b)] = qk[cp[t]];
            }
        } else {
            const int i = r - nc, b = rp[i];
            if (lane == 0) {
                oci[ob] = blocks[i];
                ova[ob] = qk[i];
                of[r] = f[i];
            }
            for (int t = b + lane; t < rp[i + 1]; t += 64) {
                oci[ob + 1 + (t - b)] = nc + ci[t];
                ova[ob + 1 + (t - b)] = va[t];
            }
        }
    }
}
__global__ void k_aug_back(int M, int n, int nc, const int* __restrict__ blocks,
                           const double* __restrict__ U, const double* __restrict__ p,
                           const double* __restrict__ q, double* __restrict__ zeta) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const double qp = i < n ? q[i] : -p[i - n];
        zeta[i] = qp * (U[blocks[i]] + U[nc + i]);              // :35-36
    }
}

void aug_pcg_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, double tol, long long maxit, double* zeta,
                 HybridOut* out) {
    IPD_REQUIRE(sys.tk != 0.0, IPD_E_ARG, "tk must be nonzero");
    const int n = sys.n, M = sys.M();
    const double *p = sys.p, *q = sys.q;
    Arena& tmp = *ctx->scratch;
    Csr Ae;
    build_Ae(ctx, tmp, sys, &Ae);
    double* f = tmp.alloc<double>((size_t)M);
    const int g = elems_grid(M);
    scale_qp(ctx, sys, z, f);
    Components cc;
    find_components(ctx, sys.H0, &cc);                                              // :24
    const int nc = cc.ncomp;
    int* d_cr = tmp.alloc<int>((size_t)nc + 1);
    int* d_cp = tmp.alloc<int>((size_t)M);
    int* d_bl = tmp.alloc<int>((size_t)M);
    ctx->upload(d_cr, cc.r.data(), (size_t)nc + 1);
    ctx->upload(d_cp, cc.p.data(), (size_t)M);
    ctx->upload(d_bl, cc.blocks.data(), (size_t)M);
    double* qk = tmp.alloc<double>((size_t)M);
    hipLaunchKernelGGL(k_aug_qk, dim3(g), dim3(256), 0, ctx->stream, M, n, p, q, sys.tdiag, sys.bk1, 1.0 / sys.tk, qk);
    Csr aug;
    aug.nr = aug.nc = nc + M;
    int* len = tmp.alloc<int>((size_t)aug.nr + 1);
    aug.rp = tmp.alloc<int>((size_t)aug.nr + 1);
    hipLaunchKernelGGL(k_aug_rowlen, dim3(elems_grid(aug.nr)), dim3(256), 0, ctx->stream, nc, M,
                       (const int*)d_cr, (const int*)Ae.rp, len);
    IPD_KERNEL_CHECK();
    aug.nnz = exclusive_scan_total(ctx, len, aug.rp, aug.nr);
    aug.ci = tmp.alloc<int>((size_t)aug.nnz);
    aug.va = tmp.alloc<double>((size_t)aug.nnz);
    double* augf = tmp.alloc<double>((size_t)aug.nr);
    double* U = tmp.alloc<double>((size_t)aug.nr);
    hipLaunchKernelGGL(k_aug_fill, dim3(rows_grid(aug.nr)), dim3(256), 0, ctx->stream, nc, M,
                       (const int*)d_cr, (const int*)d_cp, (const int*)d_bl, (const double*)qk,
                       (const double*)f, (const int*)Ae.rp, (const int*)Ae.ci, (const double*)Ae.va,
                       (const int*)aug.rp, aug.ci, aug.va, augf);
    IPD_KERNEL_CHECK();
    long long it = 0;
    double res = 0.0;
    pcg_dev(ctx, aug, augf, nullptr, tol, maxit, 2, U, &it, &res, nullptr);         // :29-34
    hipLaunchKernelGGL(k_aug_back, dim3(g), dim3(256), 0, ctx->stream, M, n, nc, (const int*)d_bl,
                       (const double*)U, p, q, zeta);
    IPD_KERNEL_CHECK();
    out->itamg = (int)std::min<long long>(it, 2147483647LL);
    out->resamg = res;
    out->num_comp = nc;
    out->it_num = 1;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
// [zeta,itpcg,respcg,info] = aug_PCG(prob_data,pcg_options) (aug_PCG.m:1) and
// PCG4POT(prob_data,pcg_options) (Class2/PCG4POT.m:1); precd is forced to 2 (aug_PCG.m:32)
static int aug_host(ipd_ctx* ctx, const ipd_prob* pd, const ipd_pcg_opts* o, bool pot, double* zeta,
                    int64_t* itpcg, double* respcg, int64_t info[2]) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && zeta, IPD_E_ARG, "NULL argument");
        const double tol = (o && o->retol >= 0) ? o->retol : 1e-11;                 // PCG.m:25-26
        const long long maxit = (o && o->maxit >= 0) ? o->maxit : 10000;
        CallScope scope(ctx);
        CompOrderScope order_scope(ctx);
        const ProbDev d = upload_prob(ctx, pd, pot);
        HybridOut ho;
        if (pot)
            pcg4pot_dev(ctx, d.sys, d.z, d.s, d.phi, tol, maxit, d.zeta, &ho);
        else
            aug_pcg_dev(ctx, d.sys, d.z, tol, maxit, d.zeta, &ho);
        ctx->fetch(d.zeta, zeta, d.len);
        report(ho, itpcg, respcg, info);
    });
}
extern "C" int ipd_aug_pcg(ipd_ctx* ctx, const ipd_prob* pd, const ipd_pcg_opts* o, double* zeta,
                           int64_t* itpcg, double* respcg, int64_t info[2]) {
    return aug_host(ctx, pd, o, false, zeta, itpcg, respcg, info);
}
extern "C" int ipd_pcg4pot(ipd_ctx* ctx, const ipd_prob* pd, const ipd_pcg_opts* o, double* zeta,
                           int64_t* itpcg, double* respcg, int64_t info[2]) {
    return aug_host(ctx, pd, o, true, zeta, itpcg, respcg, info);
}
