// The Newton system of the problem-level solvers on the device: Ae (Hybrid_AMG.m:17-24), Jk
// (APD_SsN_Class1.m:151), the sub-matrix of a component, and the vector helpers that go with them.
//
// Ae = bk1*Q0^2 + (Q0*T*Q0 + Q0*H0*Q0)/tk is assembled entry by entry with the
// reference's operation order (no FMA), so it is bit-identical to the oracle's and
// the hierarchy built on it stays bit-exact.
#pragma clang fp contract(off)

#include "ipd_hybrid_state.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// prob_data of the host ABI
// ---------------------------------------------------------------------------
template <class T>
static T* uploaded(ipd_ctx* ctx, const T* src, size_t cnt) {
    T* dst = ctx->scratch->alloc<T>(cnt);
    ctx->upload(dst, src, cnt);
    return dst;
}
ProbDev upload_prob(ipd_ctx* ctx, const ipd_prob* pd, bool pot) {
    IPD_REQUIRE(pd && pd->p && pd->q && pd->H0 && pd->z, IPD_E_ARG, "prob_data: NULL field");
    IPD_REQUIRE(pd->m > 0 && pd->n > 0 && pd->m + pd->n < (int64_t(1) << 30), IPD_E_ARG,
                "prob_data: bad m/n");
    if (pot) IPD_REQUIRE(pd->s && pd->phi, IPD_E_ARG, "AMG4POT needs prob_data.s and .phi");
    Arena& tmp = *ctx->scratch;
    ProbDev d;
    NewtonSys& sys = d.sys;
    sys.m = (int)pd->m;
    sys.n = (int)pd->n;
    sys.bk1 = pd->bk1;
    sys.tk = pd->tk;
    const size_t M = (size_t)sys.M(), mn = (size_t)sys.m * sys.n;
    d.len = M + (pot ? 1 : 0);
    csr_upload_from_csc(ctx, tmp, pd->H0, true, &sys.H0);
    sys.p = uploaded(ctx, pd->p, (size_t)sys.m);
    sys.q = uploaded(ctx, pd->q, (size_t)sys.n);
    d.z = uploaded(ctx, pd->z, d.len);
    if (pot) {
        d.phi = uploaded(ctx, pd->phi, mn);
        d.s = uploaded(ctx, pd->s, mn);
    }
    if (pd->t) sys.tdiag = uploaded(ctx, pd->t, M);
    d.zeta = tmp.alloc<double>(d.len);
    return d;
}

// ---------------------------------------------------------------------------
// Ae assembly                                             (Hybrid_AMG.m:17-24)
// ---------------------------------------------------------------------------
__device__ __forceinline__ double qp_of(const double* __restrict__ p, const double* __restrict__ q,
                                        int n, int i) {
    return i < n ? q[i] : -p[i - n];  // qp = [q; -p]
}

// row lengths of Ae: the pattern of H0 plus a full diagonal; flags a zero in p or q (Hybrid_AMG.m:18-19); the last
// workgroup scans the lengths into Ae's row pointers and posts total and flag to the host
__global__ __launch_bounds__(256) void k_ae_count(int M, int n, const int* __restrict__ rp,
                                                  const int* __restrict__ ci, const double* __restrict__ p,
                                                  const double* __restrict__ q, int* rowlen,
                                                  const ScanTail st) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int i = wave; i < M; i += nwaves) {
        bool has = false;
        for (int t = rp[i] + lane; t < rp[i + 1]; t += 64) has |= (ci[t] == i);
        const bool hasd = __any(has);
        if (lane == 0)
            scan_put(rowlen, i, rp[i + 1] - rp[i] + (hasd ? 0 : 1), (i < n ? q[i] : p[i - n]) == 0.0);
    }
    scan_tail(st);
}

__global__ __launch_bounds__(256) void k_ae_fill(int M, int n, const int* __restrict__ rp,
                                                 const int* __restrict__ ci,
                                                 const double* __restrict__ va,
                                                 const double* __restrict__ p,
                                                 const double* __restrict__ q,
                                                 const double* __restrict__ tdiag, double bk1,
                                                 double inv_tk, const int* __restrict__ orp,
                                                 int* __restrict__ oci, double* __restrict__ ova) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int i = wave; i < M; i += nwaves) {
        const int b = rp[i], e = rp[i + 1];
        const double qi = qp_of(p, q, n, i);
        // number of stored columns below i, and whether the diagonal is stored
        int below = 0;
        bool has = false;
        for (int t = b + lane; t < e; t += 64) {
            const int j = ci[t];
            below += (j < i);
            has |= (j == i);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) below += __shfl_xor(below, d);
        has = __any(has);
        const int ob = orp[i];
        const int shift = has ? 0 : 1;
        for (int t = b + lane; t < e; t += 64) {
            const int j = ci[t];
            const double a0 = (qi * va[t]) * qp_of(p, q, n, j);  // (Q0*H0)*Q0
            const int pos = ob + (t - b) + (j > i ? shift : 0);
            oci[pos] = j;
            if (j == i) {
                const double qq = qi * qi;                       // Q = Q0*Q0
                const double kk = tdiag ? (qi * tdiag[i]) * qi : 0.0;  // K = (Q0*T)*Q0
                const double x = kk + a0;                        // K + A0
                ova[pos] = bk1 * qq + inv_tk * x;
            } else {
                ova[pos] = inv_tk * a0;
            }
        }
        if (!has && lane == 0) {
            const double qq = qi * qi;
            const double kk = tdiag ? (qi * tdiag[i]) * qi : 0.0;
            oci[ob + below] = i;
            ova[ob + below] = bk1 * qq + inv_tk * kk;
        }
    }
}

// f = Q0*z, dK = diag(K), and zeta = Q0*u at the end
__global__ void k_scale_qp(int M, int n, const double* __restrict__ p, const double* __restrict__ q,
                           const double* __restrict__ in, double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x)
        out[i] = qp_of(p, q, n, i) * in[i];
}
__global__ void k_dk(int M, int n, const double* __restrict__ p, const double* __restrict__ q,
                     const double* __restrict__ tdiag, double* __restrict__ dK) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < M; i += gridDim.x * blockDim.x) {
        const double qi = qp_of(p, q, n, i);
        dK[i] = tdiag ? (qi * tdiag[i]) * qi : 0.0;
    }
}
void build_Ae(ipd_ctx* ctx, Arena& dst, const NewtonSys& sys, Csr* Ae) {
    const Csr& H0 = sys.H0;
    const int M = sys.M();
    IPD_REQUIRE(H0.nr == M && H0.nc == M, IPD_E_ARG, "Hybrid_AMG: H0 must be (n+m) x (n+m)");
    int* rowlen = zeroed<int>(ctx, (size_t)M + 1);   // (biased counts: see ScanTail)
    Csr a;
    a.nr = a.nc = M;
    a.rp = dst.alloc<int>((size_t)M + 1);
    TailTotal tt(ctx, rowlen, a.rp, M);   // entry count and the "p or q has a zero" flag in one message
    hipLaunchKernelGGL(k_ae_count, dim3(rows_grid(M)), dim3(256), 0, ctx->stream, M, sys.n, H0.rp, H0.ci, sys.p,
                       sys.q, rowlen, tt.t);
    IPD_KERNEL_CHECK();
    int h2[2] = {0, 0};
    tt.wait(h2);
    a.nnz = h2[0];
    IPD_REQUIRE(h2[1] == 0, IPD_E_ARG, "p or q contains 0 !!!!!");  // Hybrid_AMG.m:18-19
    a.ci = dst.alloc<int>((size_t)a.nnz);
    a.va = dst.alloc<double>((size_t)a.nnz);
    const double inv_tk = 1.0 / sys.tk;
    hipLaunchKernelGGL(k_ae_fill, dim3(rows_grid(M)), dim3(256), 0, ctx->stream, M, sys.n, H0.rp, H0.ci,
                       H0.va, sys.p, sys.q, sys.tdiag, sys.bk1, inv_tk, a.rp, a.ci, a.va);
    IPD_KERNEL_CHECK();
    *Ae = a;
}
void scale_qp(ipd_ctx* ctx, const NewtonSys& sys, const double* in, double* out) {
    const int M = sys.M();
    hipLaunchKernelGGL(k_scale_qp, dim3(elems_grid(M)), dim3(256), 0, ctx->stream, M, sys.n, sys.p, sys.q, in, out);
    IPD_KERNEL_CHECK();
}
void diag_k(ipd_ctx* ctx, const NewtonSys& sys, double* dK) {
    const int M = sys.M();
    hipLaunchKernelGGL(k_dk, dim3(elems_grid(M)), dim3(256), 0, ctx->stream, M, sys.n, sys.p, sys.q, sys.tdiag, dK);
    IPD_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// sub-matrix of one component: Aek = Ae(pk,pk), pk ascending
// ---------------------------------------------------------------------------
__global__ void k_sub_count(int nk, const int* __restrict__ pk, const int* __restrict__ rp,
                            int* __restrict__ rowlen) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nk; r += gridDim.x * blockDim.x) {
        const int i = pk[r];
        rowlen[r] = rp[i + 1] - rp[i];
    }
}
__global__ __launch_bounds__(256) void k_sub_fill(int nk, const int* __restrict__ pk,
                                                  const int* __restrict__ newidx,
                                                  const int* __restrict__ rp,
                                                  const int* __restrict__ ci,
                                                  const double* __restrict__ va,
                                                  const int* __restrict__ orp,
                                                  int* __restrict__ oci, double* __restrict__ ova) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int r = wave; r < nk; r += nwaves) {
        const int i = pk[r];
        const int b = rp[i], ob = orp[r];
        for (int t = b + lane; t < rp[i + 1]; t += 64) {
            oci[ob + (t - b)] = newidx[ci[t]];  // a component is closed: every column is inside
            ova[ob + (t - b)] = va[t];
        }
    }
}
__global__ void k_gather(int nk, const int* __restrict__ pk, const double* __restrict__ src,
                         double* __restrict__ dst) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nk; r += gridDim.x * blockDim.x)
        dst[r] = src[pk[r]];
}
__global__ void k_scatter(int nk, const int* __restrict__ pk, const double* __restrict__ src,
                          double* __restrict__ dst) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < nk; r += gridDim.x * blockDim.x)
        dst[pk[r]] = src[r];
}
ComponentCutter::ComponentCutter(ipd_ctx* c, const Csr& A)
    : ctx(c), Ae(A), newidx((size_t)A.nr), d_new(c->scratch->alloc<int>((size_t)A.nr)) {}

const int* ComponentCutter::cut(const int* pk, int nk, Csr* out) {
    Arena& tmp = *ctx->scratch;
    int* d_pk = tmp.alloc<int>((size_t)nk);   // per component: a scatter through it may run later
    std::fill(newidx.begin(), newidx.end(), -1);
    for (int r = 0; r < nk; ++r) newidx[(size_t)pk[r]] = r;
    ctx->upload(d_pk, pk, (size_t)nk);
    ctx->upload(d_new, newidx.data(), newidx.size());
    Csr Ak;
    Ak.nr = Ak.nc = nk;
    int* rowlen = tmp.alloc<int>((size_t)nk + 1);
    Ak.rp = tmp.alloc<int>((size_t)nk + 1);
    hipLaunchKernelGGL(k_sub_count, dim3(elems_grid(nk)), dim3(256), 0, ctx->stream, nk,
                       d_pk, Ae.rp, rowlen);
    IPD_KERNEL_CHECK();
    Ak.nnz = exclusive_scan_total(ctx, rowlen, Ak.rp, nk);
    Ak.ci = tmp.alloc<int>((size_t)Ak.nnz);
    Ak.va = tmp.alloc<double>((size_t)Ak.nnz);
    hipLaunchKernelGGL(k_sub_fill, dim3(rows_grid(nk)), dim3(256), 0, ctx->stream, nk, d_pk,
                       d_new, Ae.rp, Ae.ci, Ae.va, Ak.rp, Ak.ci, Ak.va);
    *out = Ak;
    return d_pk;
}
void gather_dev(ipd_ctx* ctx, int nk, const int* pk, const double* src, double* dst) {
    hipLaunchKernelGGL(k_gather, dim3(elems_grid(nk)), dim3(256), 0, ctx->stream, nk, pk, src, dst);
    IPD_KERNEL_CHECK();
}
void scatter_dev(ipd_ctx* ctx, int nk, const int* pk, const double* src, double* dst) {
    hipLaunchKernelGGL(k_scatter, dim3(elems_grid(nk)), dim3(256), 0, ctx->stream, nk, pk, src, dst);
    IPD_KERNEL_CHECK();
}

double host_sum(ipd_ctx* ctx, const double* d, int n) {
    std::vector<double> h((size_t)n);
    ctx->fetch(d, h.data(), (size_t)n);
    double s = 0.0;
    for (double v : h) s += v;
    return s;
}
double host_dot(ipd_ctx* ctx, const double* a, const double* b, int n) {
    std::vector<double> ha((size_t)n), hb((size_t)n);
    ctx->fetch(a, ha.data(), (size_t)n);
    ctx->fetch(b, hb.data(), (size_t)n);
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += ha[(size_t)i] * hb[(size_t)i];
    return s;
}

// ---------------------------------------------------------------------------
// Jk = bk1*I + (T + H0)/tk                              (APD_SsN_Class1.m:151)
// ---------------------------------------------------------------------------
// H0 stores a diagonal entry only on rows that have active entries, Jk on every row.
__global__ void k_jk_count(int M, const int* __restrict__ rp, const int* __restrict__ ci,
                           int* __restrict__ len) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < M; r += gridDim.x * blockDim.x) {
        bool has = false;
        for (int t = rp[r]; t < rp[r + 1]; ++t) has = has || ci[t] == r;
        len[r] = rp[r + 1] - rp[r] + (has ? 0 : 1);
    }
}
__global__ void k_jk_fill(int M, const int* __restrict__ rp, const int* __restrict__ ci,
                          const double* __restrict__ va, const double* __restrict__ t, double bk1,
                          double tk, const int* __restrict__ orp, int* __restrict__ oci,
                          double* __restrict__ ova) {
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < M; r += gridDim.x * blockDim.x) {
        int o = orp[r];
        bool placed = false;
        const double tr = t ? t[r] : 0.0;
        for (int k = rp[r]; k < rp[r + 1]; ++k) {
            const int c = ci[k];
            if (!placed && c > r) {   // the missing diagonal goes in before the first larger column
                oci[o] = r;
                ova[o++] = bk1 + (tr + 0.0) / tk;
                placed = true;
            }
            oci[o] = c;
            if (c == r) {
                ova[o++] = bk1 + (tr + va[k]) / tk;
                placed = true;
            } else {
                ova[o++] = va[k] / tk;
            }
        }
        if (!placed) {
            oci[o] = r;
            ova[o] = bk1 + (tr + 0.0) / tk;
        }
    }
}
void build_jk(ipd_ctx* ctx, Arena& dst, const NewtonSys& sys, Csr* J) {
    const Csr& H0 = sys.H0;
    const int M = H0.nr;
    int* len = ctx->scratch->alloc<int>((size_t)M + 1);
    J->nr = J->nc = M;
    J->rp = dst.alloc<int>((size_t)M + 1);
    hipLaunchKernelGGL(k_jk_count, dim3(elems_grid(M)), dim3(256), 0, ctx->stream, M, H0.rp, H0.ci, len);
    IPD_KERNEL_CHECK();
    J->nnz = exclusive_scan_total(ctx, len, J->rp, M);
    J->ci = dst.alloc<int>((size_t)J->nnz);
    J->va = dst.alloc<double>((size_t)J->nnz);
    hipLaunchKernelGGL(k_jk_fill, dim3(elems_grid(M)), dim3(256), 0, ctx->stream, M, H0.rp, H0.ci,
                       H0.va, sys.tdiag, sys.bk1, sys.tk, (const int*)J->rp, J->ci, J->va);
    IPD_KERNEL_CHECK();
}
