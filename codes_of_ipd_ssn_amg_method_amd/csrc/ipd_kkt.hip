// Matrix-free A operators and the closed-form inverses (the assembly ASAt is ipd_asat.hip):
//   Ax.m:10-13, Aty.m:10-13, invAAt.m:13-20, Class2/invHHt.m:7-17.
//
// Layout: x, phi are m*n column-major (X(i,j) = x[i + j*m]); the KKT unknowns
// are ordered [0,n) = column constraints, [n,n+m) = row constraints
// (Class1/APD_SsN_Class1.m:33).
//
// Roofline: all of these are single streaming passes -> HBM bound.
//   Ax   : 8*m*n + 16*(m+n) bytes      Aty : 8*m*n + 16*(m+n) bytes
// This TU is compiled with -ffp-contract=off so that Aty is bit-identical to the
// oracle (two multiplies and one add per entry).
// Grids, scratch sizes and the vec2 predicate: ipd_kkt_plan.h; tile constants: ipd_limits.h.
#pragma clang fp contract(off)

#include "ipd_kkt.h"

// ---------------------------------------------------------------------------
// Ax:  y = [X'*p ; X*q]
// ---------------------------------------------------------------------------
// A workgroup stages a 256-row x 16-column tile of X in LDS with coalesced
// column-contiguous loads (16 independent 8-byte loads in flight per lane), then
// forms 256 partial row sums (row i over the 16 columns) and 16 partial column
// sums (column j over the 256 rows) from the LDS copy.  Partials are combined
// by a second kernel in a fixed order (deterministic, no float atomics).
__global__ __launch_bounds__(256) void k_ax_tiles(const double* __restrict__ x,
                                                  const double* __restrict__ p,
                                                  const double* __restrict__ q, int m, int n,
                                                  double* __restrict__ lpart,
                                                  double* __restrict__ rpart) {
    __shared__ double tile[AX_TC * AX_LD];
    const int tid = threadIdx.x;
    const int ib = blockIdx.x, jb = blockIdx.y;
    const int i = ib * AX_TR + tid;
    const int j0 = jb * AX_TC;
    const bool in_i = i < m;
    double xv[AX_TC];
#pragma unroll
    for (int jj = 0; jj < AX_TC; ++jj) {
        const int j = j0 + jj;
        xv[jj] = (in_i && j < n) ? x[(size_t)j * m + i] : 0.0;
    }
    double lacc = 0.0;
#pragma unroll
    for (int jj = 0; jj < AX_TC; ++jj) {
        const int j = j0 + jj;
        const double qj = j < n ? q[j] : 0.0;
        lacc += xv[jj] * qj;
        tile[jj * AX_LD + tid] = xv[jj];
    }
    if (in_i) lpart[(size_t)jb * m + i] = lacc;
    __syncthreads();
    // column sums: 16 lanes per column, each lane 16 rows, then a 16-lane reduce
    const int jj = tid >> 4, sub = tid & 15;
    double cacc = 0.0;
#pragma unroll
    for (int k = 0; k < AX_TR / 16; ++k) {
        const int r = sub + 16 * k;
        const int gi = ib * AX_TR + r;
        const double pi = gi < m ? p[gi] : 0.0;
        cacc += tile[jj * AX_LD + r] * pi;
    }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) cacc += __shfl_xor(cacc, d);
    if (sub == 0 && j0 + jj < n) rpart[(size_t)ib * n + j0 + jj] = cacc;
}

// partial sums combined in ascending tile order; eight loads in flight per trip (a load per
// trip made this a chain of 64 L2 round trips: 11 us at m=n=1024 against 5 for the tiles)
__device__ __forceinline__ double ax_sum_strided(const double* __restrict__ part, int count,
                                                 size_t stride, int col) {
    double s = 0.0;
    for (int b0 = 0; b0 < count; b0 += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int b = b0 + u;
            v[u] = part[(size_t)(b < count ? b : 0) * stride + col];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (b0 + u < count) s += v[u];
    }
    return s;
}

__global__ __launch_bounds__(256) void k_ax_final(const double* __restrict__ lpart,
                                                  const double* __restrict__ rpart, int m, int n,
                                                  int nib, int njb, double* __restrict__ y) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n)
        y[t] = ax_sum_strided(rpart, nib, (size_t)n, t);
    else if (t < n + m)
        y[t] = ax_sum_strided(lpart, njb, (size_t)m, t - n);
}

void kkt_ax(ipd_ctx* ctx, const double* x, const double* p, const double* q, int m, int n,
            double* y) {
    if (m <= 0 || n <= 0) return;
    Arena& tmp = *ctx->scratch;
    const AxGeo g = ax_geo(m, n);
    double* lpart = tmp.alloc<double>(g.lpart);
    double* rpart = tmp.alloc<double>(g.rpart);
    hipLaunchKernelGGL(k_ax_tiles, dim3(g.nib, g.njb), dim3(256), 0, ctx->stream, x, p, q, m, n, lpart,
                       rpart);
    IPD_KERNEL_CHECK();
    hipLaunchKernelGGL(k_ax_final, dim3(g.final_grid), dim3(256), 0, ctx->stream, lpart, rpart,
                       m, n, g.nib, g.njb, y);
    IPD_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// Aty:  z(i,j) = p_i*y1_j + y2_i*q_j        (pure streaming write)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_aty_v2(const double* __restrict__ y,
                                                const double* __restrict__ p,
                                                const double* __restrict__ q, int m, int n,
                                                double* __restrict__ z) {
    // two consecutive rows per lane -> 16-byte stores (m even, z 16-byte aligned)
    const int i = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= m) return;
    const double p0 = p[i], p1 = p[i + 1];
    const double a0 = y[n + i], a1 = y[n + i + 1];
    const int j0 = blockIdx.y * ATY_TC;
#pragma unroll
    for (int jj = 0; jj < ATY_TC; ++jj) {
        const int j = j0 + jj;
        if (j < n) {
            const double y1 = y[j], qj = q[j];
            double2 v;
            v.x = p0 * y1 + a0 * qj;
            v.y = p1 * y1 + a1 * qj;
            *reinterpret_cast<double2*>(z + (size_t)j * m + i) = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_aty_v1(const double* __restrict__ y,
                                                const double* __restrict__ p,
                                                const double* __restrict__ q, int m, int n,
                                                double* __restrict__ z) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double pi = p[i], ai = y[n + i];
    const int j0 = blockIdx.y * ATY_TC;
#pragma unroll
    for (int jj = 0; jj < ATY_TC; ++jj) {
        const int j = j0 + jj;
        if (j < n) z[(size_t)j * m + i] = pi * y[j] + ai * q[j];
    }
}

void kkt_aty(ipd_ctx* ctx, const double* y, const double* p, const double* q, int m, int n,
             double* z) {
    if (m <= 0 || n <= 0) return;
    const bool vec2 = aty_vec2(m, reinterpret_cast<uintptr_t>(z));
    hipLaunchKernelGGL(vec2 ? k_aty_v2 : k_aty_v1, dim3(aty_grid_x(m, vec2), aty_grid_y(n)), dim3(256), 0, ctx->stream,
                       y, p, q, m, n, z);
    IPD_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// invAAt / invHHt  (closed forms; O(m+n) plus one Ax for invHHt)
// ---------------------------------------------------------------------------
__device__ inline double block_sum_1024(double v, double* red) {
    // all 1024 threads participate; returns the sum in every thread
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k];
    return s;
}

// y = (diag(sg1 I_n, sg2 I_m) + A A')^{-1} x        invAAt.m:13-20
__global__ __launch_bounds__(1024) void k_inv_aat(const double* __restrict__ x,
                                                  const double* __restrict__ p,
                                                  const double* __restrict__ q, int m, int n,
                                                  double sg1, double sg2, double* __restrict__ y) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    double a = 0, b = 0, c = 0, d = 0;
    for (int i = tid; i < m; i += 1024) {
        a += p[i] * p[i];
        c += p[i] * x[n + i];
    }
    for (int j = tid; j < n; j += 1024) {
        b += q[j] * q[j];
        d += q[j] * x[j];
    }
    const double np = block_sum_1024(a, red);
    const double nq = block_sum_1024(b, red);
    const double pvm = block_sum_1024(c, red);
    const double qvn = block_sum_1024(d, red);
    const double den = sg1 * sg2 + sg1 * nq + sg2 * np;
    const double cn = (np / (sg1 + np) * qvn - pvm);
    const double cm = (nq / (sg2 + nq) * pvm - qvn);
    for (int j = tid; j < n; j += 1024) y[j] = x[j] / (sg1 + np) + cn * q[j] / den;
    for (int i = tid; i < m; i += 1024) y[n + i] = x[n + i] / (sg2 + nq) + cm * p[i] / den;
}

void kkt_inv_aat(ipd_ctx* ctx, const double* x, const double* p, const double* q, int m, int n,
                 double sg1, double sg2, double* y) {
    hipLaunchKernelGGL(k_inv_aat, dim3(1), dim3(1024), 0, ctx->stream, x, p, q, m, n, sg1, sg2, y);
    IPD_KERNEL_CHECK();
}

__global__ __launch_bounds__(256) void k_sumsq_partial(const double* __restrict__ v, size_t len,
                                                       double* __restrict__ part) {
    __shared__ double red[4];
    double a = 0.0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < len; i += (size_t)gridDim.x * 256)
        a += v[i] * v[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Class2/invHHt.m:8-17 once l = Ax(phi), Vl = invAAt(l,sg+1), Vv1 = invAAt(v1,sg+1)
__global__ __launch_bounds__(1024) void k_inv_hht_combine(const double* __restrict__ v,
                                                          const double* __restrict__ l,
                                                          const double* __restrict__ Vl,
                                                          const double* __restrict__ Vv1,
                                                          const double* __restrict__ part,
                                                          int npart, int M, double sg,
                                                          double* __restrict__ y) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    double a = 0, b = 0, c = 0;
    for (int k = tid; k < npart; k += 1024) a += part[k];
    for (int k = tid; k < M; k += 1024) {
        b += l[k] * Vl[k];
        c += l[k] * Vv1[k];
    }
    const double t = sg + block_sum_1024(a, red);
    const double lVl = block_sum_1024(b, red);
    const double lVv = block_sum_1024(c, red);
    const double s = t - lVl;
    const double v2 = v[M];
    for (int k = tid; k < M; k += 1024) y[k] = (s * Vv1[k] + lVv * Vl[k] - v2 * Vl[k]) / s;
    if (tid == 0) y[M] = (v2 - lVv) / s;
}

void kkt_inv_hht_pre(ipd_ctx* ctx, const double* v, const double* p, const double* q, int m, int n,
                     double sg, const double* l, const double* part, int npart, double* y) {
    Arena& tmp = *ctx->scratch;
    const int M = m + n;
    double* Vl = tmp.alloc<double>((size_t)M);
    double* Vv1 = tmp.alloc<double>((size_t)M);
    kkt_inv_aat(ctx, l, p, q, m, n, sg + 1, sg + 1, Vl);
    kkt_inv_aat(ctx, v, p, q, m, n, sg + 1, sg + 1, Vv1);
    hipLaunchKernelGGL(k_inv_hht_combine, dim3(1), dim3(1024), 0, ctx->stream, v, l, Vl, Vv1, part,
                       npart, M, sg, y);
    IPD_KERNEL_CHECK();
}

int kkt_phi_consts(ipd_ctx* ctx, const double* phi, const double* p, const double* q, int m, int n,
                   double* l, double* part) {
    const int npart = phi_parts(m, n);
    hipLaunchKernelGGL(k_sumsq_partial, dim3(npart), dim3(256), 0, ctx->stream, phi, (size_t)m * n, part);
    IPD_KERNEL_CHECK();
    kkt_ax(ctx, phi, p, q, m, n, l);
    return npart;
}

void kkt_inv_hht(ipd_ctx* ctx, const double* v, const double* p, const double* q, int m, int n,
                 double sg, const double* phi, double* y) {
    double* part = ctx->scratch->alloc<double>((size_t)phi_parts(m, n));
    double* l = ctx->scratch->alloc<double>((size_t)m + n);
    const int npart = kkt_phi_consts(ctx, phi, p, q, m, n, l, part);
    kkt_inv_hht_pre(ctx, v, p, q, m, n, sg, l, part, npart, y);
}

// ---------------------------------------------------------------------------
// C ABI (the frames: ipd_kkt.h)
// ---------------------------------------------------------------------------
extern "C" int ipd_ax_dev(ipd_ctx* ctx, const double* x, const double* p, const double* q,
                          int64_t m, int64_t n, double* y) {
    return kkt_dev_entry(ctx, x && p && q && y, m, n, [&](int mi, int ni) { kkt_ax(ctx, x, p, q, mi, ni, y); });
}

extern "C" int ipd_aty_dev(ipd_ctx* ctx, const double* y, const double* p, const double* q,
                           int64_t m, int64_t n, double* z) {
    return kkt_dev_entry(ctx, z && p && q && y, m, n, [&](int mi, int ni) { kkt_aty(ctx, y, p, q, mi, ni, z); });
}

static const double* f64(const void* d) { return static_cast<const double*>(d); }

extern "C" int ipd_ax(ipd_ctx* ctx, const double* x, const double* p, const double* q, int64_t m,
                      int64_t n, double* y) {
    const size_t um = (size_t)m, un = (size_t)n;
    return kkt_host_entry(ctx, {{x, 8 * um * un}}, p, q, m, n, y, um + un,
                          [&](const void* const* d, const double* dp, const double* dq, double* dy, int mi, int ni) {
                              kkt_ax(ctx, f64(d[0]), dp, dq, mi, ni, dy);
                          });
}

extern "C" int ipd_aty(ipd_ctx* ctx, const double* y, const double* p, const double* q, int64_t m,
                       int64_t n, double* z) {
    const size_t um = (size_t)m, un = (size_t)n;
    return kkt_host_entry(ctx, {{y, 8 * (um + un)}}, p, q, m, n, z, um * un,
                          [&](const void* const* d, const double* dp, const double* dq, double* dz, int mi, int ni) {
                              kkt_aty(ctx, f64(d[0]), dp, dq, mi, ni, dz);
                          });
}

extern "C" int ipd_inv_aat(ipd_ctx* ctx, const double* x, const double* p, const double* q,
                           int64_t m, int64_t n, double sg1, double sg2, double* y) {
    const size_t um = (size_t)m, un = (size_t)n;
    return kkt_host_entry(ctx, {{x, 8 * (um + un)}}, p, q, m, n, y, um + un,
                          [&](const void* const* d, const double* dp, const double* dq, double* dy, int mi, int ni) {
                              kkt_inv_aat(ctx, f64(d[0]), dp, dq, mi, ni, sg1, sg2, dy);
                          });
}

extern "C" int ipd_inv_hht(ipd_ctx* ctx, const double* v, const double* p, const double* q,
                           int64_t m, int64_t n, double sg, const double* phi, double* y) {
    const size_t um = (size_t)m, un = (size_t)n;
    return kkt_host_entry(ctx, {{v, 8 * (um + un + 1)}, {phi, 8 * um * un}}, p, q, m, n, y, um + un + 1,
                          [&](const void* const* d, const double* dp, const double* dq, double* dy, int mi, int ni) {
                              kkt_inv_hht(ctx, f64(d[0]), dp, dq, mi, ni, sg, f64(d[1]), dy);
                          });
}
