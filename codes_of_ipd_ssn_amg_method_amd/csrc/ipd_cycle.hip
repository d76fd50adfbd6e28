// Solve phase on the device: the V/W cycle, its smoothers, the coarsest-level
// Jacobi-PCG and the Class_AMG stationary iteration.
//   AMG/MG_Vcycle.m:9-45, AMG/MG_Wcycle.m:10-46, PCG.m:68-87, AMG/Class_AMG.m:86-109.
//
// Kernel design (all HBM/L2-bandwidth or latency bound; no MFMA -- sparse fp64):
//  * one CSR row walk per smoother sweep.  The reference applies an explicit
//    smoother matrix (g = r - A e; e += R g, Rk{1} = forward Gauss-Seidel on the
//    bipartite blocks, Rk{k>1} = 0.5 D^-1).  Algebraically R*(r - A e) for the
//    block-triangular Rk{1} is a forward (F then C) Gauss-Seidel half-sweep pair:
//    the second half reads the first half's result, so one pass over A per sweep
//    (S(A_1) bytes, the minimum) replaces SpMV(A)+SpMV(R).  Rk{1}' is the backward
//    (C then F) pair.
//  * the kernel-augmented smoother (isnsp, MG_Vcycle.m:15-21) needs xig = 1'(r-Ae)
//    BEFORE the sweep; we use 1'(r - A e) = 1'r - (A1)'e (A symmetric), with the
//    two sums carried as per-block partials written by whichever kernel produced
//    r and e, so no extra pass or launch is needed and the result is
//    run-to-run deterministic (no float atomics).
//  * rows are split over L lanes (4..1024) chosen per level from nnz/row so that
//    short rows do not idle a wave and long rows still fill the chip.
// Solve-phase results differ from the oracle only by summation order: tests
// compare residual histories to 1e-10.
#include "ipd_amg_internal.h"

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>

#include "ipd_cycle_dev.h"
#include "ipd_cycle_phases.h"

// Dynamic LDS = the staged gather vector (N doubles) when STAGED, else nothing.
template <bool STAGED, bool PAD>
__global__ __launch_bounds__(BT) void k_smooth(SmoothArgs a) {
    __shared__ PhaseLds lds;
    extern __shared__ __attribute__((aligned(16))) double xs_dyn[];
    phase_smooth<STAGED, PAD>(a, blockIdx.x, gridDim.x, &lds, xs_dyn);
}
template <bool STAGED, bool PAD>
__global__ __launch_bounds__(BT) void k_resid(LevelDev lv, const double* e, int row0, int row1) {
    __shared__ PhaseLds lds;
    extern __shared__ __attribute__((aligned(16))) double xs_dyn[];
    phase_resid<STAGED, PAD>(lv, e, row0, row1, blockIdx.x, gridDim.x, &lds, xs_dyn);
}
template <bool STAGED>
__global__ __launch_bounds__(BT) void k_xfer(XferArgs a) {
    __shared__ PhaseLds lds;
    extern __shared__ __attribute__((aligned(16))) double xs_dyn[];
    phase_xfer<STAGED>(a, blockIdx.x, gridDim.x, &lds, xs_dyn);
}
template <bool STAGED>
__global__ __launch_bounds__(BT) void k_rrc(RrcArgs a) {
    __shared__ PhaseLds lds;
    extern __shared__ __attribute__((aligned(16))) double xs_dyn[];
    phase_rrc<STAGED>(a, blockIdx.x, gridDim.x, &lds, xs_dyn);
}
template <bool STAGED, bool PAD>
__global__ __launch_bounds__(BT) void k_top(TopArgs a) {
    __shared__ PhaseLds lds;
    extern __shared__ __attribute__((aligned(16))) double xs_dyn[];
    phase_top<STAGED, PAD>(a, blockIdx.x, gridDim.x, &lds, xs_dyn);
}

// padded off-diagonal copy of a CSR matrix: one wave per row
__device__ __forceinline__ void pad_build_rows(int vb, int nvb, int N, int S, const int* __restrict__ rp,
                                               const int* __restrict__ ci, const double* __restrict__ va,
                                               unsigned short* __restrict__ pci, double* __restrict__ pva,
                                               double* __restrict__ diag) {
    const int lane = threadIdx.x & 63;
    const int wave = (vb * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (nvb * blockDim.x) >> 6;
    for (int r = wave; r < N; r += nwaves) {
        const int b = rp[r], e = rp[r + 1];
        int dpos = 0x7fffffff;
        for (int t = b + lane; t < e; t += 64)
            if (ci[t] == r) dpos = t;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) dpos = min(dpos, __shfl_xor(dpos, d));
        const bool hasd = dpos != 0x7fffffff;
        const size_t base = (size_t)r * S;
        for (int t = b + lane; t < e; t += 64) {
            if (t == dpos) continue;
            const int k = (t - b) - ((hasd && dpos < t) ? 1 : 0);
            pci[base + k] = (unsigned short)ci[t];
            pva[base + k] = va[t];
        }
        const int len = (e - b) - (hasd ? 1 : 0);
        for (int k = len + lane; k < S; k += 64) {
            pci[base + k] = 0;
            pva[base + k] = 0.0;
        }
        if (lane == 0) diag[r] = hasd ? va[dpos] : 0.0;
    }
}
__global__ __launch_bounds__(256) void k_pad_build(int N, int S, const int* __restrict__ rp,
                                                   const int* __restrict__ ci,
                                                   const double* __restrict__ va,
                                                   unsigned short* __restrict__ pci,
                                                   double* __restrict__ pva,
                                                   double* __restrict__ diag) {
    pad_build_rows(blockIdx.x, gridDim.x, N, S, rp, ci, va, pci, pva, diag);
}
// the padded copies of all the levels of a hierarchy in one launch (blockIdx.y = entry)
constexpr int PAD_BATCH = 8;
struct PadBatch {
    int n = 0;
    int N[PAD_BATCH], S[PAD_BATCH];
    const int* rp[PAD_BATCH];
    const int* ci[PAD_BATCH];
    const double* va[PAD_BATCH];
    unsigned short* pci[PAD_BATCH];
    double* pva[PAD_BATCH];
    double* diag[PAD_BATCH];
};
__global__ __launch_bounds__(256) void k_pad_build_batch(const PadBatch b) {
    const int q = blockIdx.y;
    pad_build_rows(blockIdx.x, gridDim.x, b.N[q], b.S[q], b.rp[q], b.ci[q], b.va[q], b.pci[q], b.pva[q], b.diag[q]);
}

// hist[0] = res0 (set on the first call), hist[1] = res, hist[2] = previous res,
// hist[3] = rel_res, hist[4] = rhok                        Class_AMG.m:89,103-105
struct ConvArgs {
    const double* r;
    int n;
    double* hist;
    int first;
};

__device__ __forceinline__ void conv_block(const ConvArgs& a, double* red) {
    double s = 0.0;
    for (int k0 = threadIdx.x; k0 < a.n; k0 += 4 * BT) {  // 4 independent loads in flight
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * BT;
            v[u] = a.r[k < a.n ? k : a.n - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s += (k0 + u * BT < a.n) ? v[u] * v[u] : 0.0;
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) {
        double* hist = a.hist;
        const double res = sqrt(tot);
        if (a.first) {
            hist[0] = res;
            hist[1] = res;
            hist[2] = res;
            hist[3] = 1.0;
            hist[4] = 0.0;
        } else {
            const double prev = hist[1];
            hist[2] = prev;
            hist[1] = res;
            hist[3] = res / hist[0];
            hist[4] = res / prev;
        }
    }
}

// sum of a vector into one slot (entry point of ipd_amg_vcycle / wcycle)
__global__ __launch_bounds__(BT) void k_vec_sum(const double* v, int n, double* out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += BT) s += v[k];
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = tot;
}

__global__ __launch_bounds__(BT) void k_dot_sum(const double* a, const double* b, int n,
                                                double* out) {
    __shared__ double red[16];
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += BT) s += a[k] * b[k];
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) out[0] = tot;
}

// ---------------------------------------------------------------------------
// PCG (Shewchuk B3) in one workgroup                              PCG.m:68-87
// ---------------------------------------------------------------------------
// The hot use is the coarsest level (N <= 1+fix(M^(1/3)), i.e. <= 17 rows): the
// whole solve is latency, so it runs inside one workgroup with no host round
// trips.  Vectors live in global scratch (L1/L2 resident).  precd: 1 none, 2 Jacobi.
struct PcgArgs {
    int N, L;
    const int* rp;
    const int* ci;
    const double* va;
    const double* rhs;
    const double* guess;  // NULL -> zeros
    double* d;            // solution
    double* work;         // 4*N doubles: r, p, q, diag
    double tol;
    long long maxit;
    int precd;
    double* out;          // out[0] = it, out[1] = res ; then resk[0..min(it,nresk))
    long long nresk;
};

// A 1x1 coarsest level (dense masks: levels 2048 / 1024 / 1) through the block-wide reductions
// costs ~10 us per cycle for five multiplications; one thread runs the same recurrence in
// registers.  Every block sum of the general path has a single nonzero term here, so the bits
// are the same.
__device__ __forceinline__ void pcg_single(const PcgArgs& a) {
    if (threadIdx.x == 0) {
        double h = 0.0;   // H(1,1); a structurally empty row leaves it 0 as the general path does
        for (int t = a.rp[0]; t < a.rp[1]; ++t)
            if (a.ci[t] == 0) h = a.va[t];
        const double g0 = a.guess ? a.guess[0] : 0.0;
        double r = a.rhs[0] - (a.guess ? h * g0 : 0.0);                         // :68
        double p = a.precd == 2 ? r / h : r;
        double d = g0;
        double delta_new = r * p;
        const double delta_0 = delta_new, thresh = a.tol * a.tol * delta_0;
        long long it = 0;
        while (it < a.maxit && delta_new > thresh) {                            // :76
            const double delta_old = delta_new;
            const double q = h * p;
            const double alpha = delta_old / (q * p);                           // :78
            d += alpha * p;
            r = r - alpha * q;                                                  // :79
            const double w = a.precd == 2 ? r / h : r;                          // :80
            delta_new = r * w;                                                  // :81
            p = w + (delta_new / delta_old) * p;                                // :82-83
            ++it;
            if (a.out && it <= a.nresk) a.out[1 + it] = sqrt(fabs(delta_new / delta_0));
        }
        a.d[0] = d;
        if (a.out) {
            a.out[0] = (double)it;
            a.out[1] = sqrt(fabs(delta_new / delta_0));
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void pcg_block(const PcgArgs& a, double* red) {
    if (a.N == 1) {
        pcg_single(a);
        return;
    }
    const int tid = threadIdx.x;
    const int N = a.N, L = a.L, gpb = BT / L;
    const int g = tid / L, gl = tid - g * L;
    double* r = a.work;
    double* p = a.work + N;
    double* q = a.work + 2 * (size_t)N;
    double* dg = a.work + 3 * (size_t)N;
    const int niter = (N + gpb - 1) / gpb;
    // r = e - H*d0 ; diag ; p = M^-1 r ; delta_new = r'p                     :68-70
    double acc = 0.0;
    for (int it = 0; it < niter; ++it) {
        const int row = it * gpb + g;
        const bool valid = row < N;
        double s = 0.0, dd = 0.0;
        if (valid)
            for (int t = a.rp[row] + gl; t < a.rp[row + 1]; t += L) {
                const int j = a.ci[t];
                if (a.guess) s += a.va[t] * a.guess[j];
                if (j == row) dd = a.va[t];
            }
        s = group_sum(s, L, red);
        dd = group_sum(dd, L, red);
        if (valid && gl == 0) {
            const double ri = a.rhs[row] - s;
            const double pi = a.precd == 2 ? ri / dd : ri;
            r[row] = ri;
            dg[row] = dd;
            p[row] = pi;
            a.d[row] = a.guess ? a.guess[row] : 0.0;
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
        for (int it = 0; it < niter; ++it) {  // q = H*p ; q'p
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
            a.d[row] += alpha * p[row];
            const double ri = r[row] - alpha * q[row];                          // :79
            r[row] = ri;
            const double wi = a.precd == 2 ? ri / dg[row] : ri;                 // :80
            q[row] = wi;  // q is free again: holds w
            acc += ri * wi;
        }
        delta_new = block_sum(acc, red);                                        // :81
        const double beta = delta_new / delta_old;                              // :82
        for (int row = tid; row < N; row += BT) p[row] = q[row] + beta * p[row];  // :83
        ++it_count;
        if (tid == 0 && a.out && it_count <= a.nresk)
            a.out[1 + it_count] = sqrt(fabs(delta_new / delta_0));              // :85
    }
    if (tid == 0 && a.out) {
        a.out[0] = (double)it_count;
        a.out[1] = sqrt(fabs(delta_new / delta_0));                             // :87 (0/0 -> NaN)
    }
    __syncthreads();
}

__global__ __launch_bounds__(BT) void k_pcg(PcgArgs a) {
    __shared__ double red[16];
    pcg_block(a, red);
}

// ---------------------------------------------------------------------------
// PCG with the triangular preconditioners of PCG.m: precd 3 (SSOR, w = 1.5, :40-44,96-99) and
// precd 5 (SSOR on the bigraph blocks, :52-62).  Cold paths (the drivers use precd 2): one
// workgroup, correctness first.  The two triangular solves of precd 3 are sequential in the row
// index: wave 0 walks the rows in order (lanes over a row's entries); the unknowns live in LDS.
// precd 5 is applied matrix-free: with y_C = T^-1 (r_C - w U' V^-1 r_F),
//     P r = w(2-w) [ V^-1 (r_F - w U y_C) ; y_C ]      (the block product of :59-60 expanded)
// ---------------------------------------------------------------------------
struct PcgGenArgs {
    PcgArgs a;
    int nf;          // precd 5: size of the F block
    double* tmp;     // 2*N doubles
    double* lva;     // precd 4: the incomplete Cholesky factor on H's pattern (nnz doubles; entries
                     // above the diagonal unused), its diagonal in ldg (N doubles)
    double* ldg;
};

// precd 4: P = ichol(H) with MATLAB's defaults -- IC(0): type 'nofill', no drop tolerance, no
// diagonal compensation (PCG.m:44-46).  L has the pattern of tril(H) and
//   L(i,k) = (H(i,k) - sum_{j<k} L(i,j) L(k,j)) / L(k,k),  L(i,i) = sqrt(H(i,i) - sum_{j<i} L(i,j)^2),
// the sums running over the common pattern.  MATLAB's kernel is closed source, so the order of the
// sums (here: ascending j) is this build's; a nonpositive pivot is MATLAB's error
// "Encountered nonpositive pivot" (*fail = 1 + row).  Rows are sequential: one wave, the current
// row scattered into the LDS array `wrow` (N doubles, all zero on entry and on exit).
__device__ __forceinline__ void pcg_ichol0(const PcgGenArgs& g, double* wrow, int* fail) {
    const PcgArgs& a = g.a;
    const int lane = threadIdx.x, N = a.N;
    for (int i = 0; i < N; ++i) {
        const int b = a.rp[i], e = a.rp[i + 1];
        double hii = 0.0;
        bool has_diag = false;
        for (int t = b; t < e; ++t) {            // entries of the row in ascending column order
            const int k = a.ci[t];
            if (k > i) break;
            if (k == i) {
                hii = a.va[t];
                has_diag = true;
                break;
            }
            double sdot = 0.0;
            for (int u = a.rp[k] + lane; u < a.rp[k + 1]; u += 64) {
                const int j = a.ci[u];
                if (j < k) sdot += g.lva[u] * wrow[j];
            }
            sdot = wave_sum(sdot);
            const double lik = (a.va[t] - sdot) / g.ldg[k];
            if (lane == 0) {
                g.lva[t] = lik;
                wrow[k] = lik;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        double sq = 0.0;
        for (int t = b + lane; t < e; t += 64) {
            const int j = a.ci[t];
            if (j < i) {
                const double l = wrow[j];
                sq += l * l;
            }
        }
        sq = wave_sum(sq);
        const double d = hii - sq;
        if (!has_diag || !(d > 0.0)) {
            if (lane == 0) *fail = 1 + i;
            return;
        }
        __builtin_amdgcn_wave_barrier();
        for (int t = b + lane; t < e; t += 64) {   // leave wrow zero for the next row
            const int j = a.ci[t];
            if (j < i) wrow[j] = 0.0;
            if (j == i) g.lva[t] = sqrt(d);
        }
        if (lane == 0) g.ldg[i] = sqrt(d);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

__device__ __forceinline__ void pcg_gen_prec(const PcgGenArgs& g, const double* r, double* w,
                                             double* sol /*LDS, N*/, double* red) {
    const PcgArgs& a = g.a;
    const int tid = threadIdx.x, N = a.N;
    const double* dg = a.work + 3 * (size_t)N;
    const double om = 1.5, c = om * (2.0 - om);
    if (a.precd == 5) {
        const int nf = g.nf;
        double* t1 = g.tmp;   // V^-1 r_F
        for (int i = tid; i < nf; i += BT) t1[i] = r[i] / dg[i];
        __syncthreads();
        for (int i = nf + tid; i < N; i += BT) {   // y_C
            double sdot = 0.0;
            for (int t = a.rp[i]; t < a.rp[i + 1]; ++t)
                if (a.ci[t] < nf) sdot += a.va[t] * t1[a.ci[t]];
            w[i] = (r[i] - om * sdot) / dg[i];
        }
        __syncthreads();
        for (int i = tid; i < nf; i += BT) {
            double sdot = 0.0;
            for (int t = a.rp[i]; t < a.rp[i + 1]; ++t)
                if (a.ci[t] >= nf) sdot += a.va[t] * w[a.ci[t]];
            w[i] = c * ((r[i] - om * sdot) / dg[i]);
        }
        __syncthreads();
        for (int i = nf + tid; i < N; i += BT) w[i] = c * w[i];
        __syncthreads();
        return;
    }
    if (a.precd == 4) {   // p = P \ r ; p = P' \ p                                PCG.m:100-101
        if (tid < 64) {
            for (int i = 0; i < N; ++i) {   // forward, rows of L
                double sdot = 0.0;
                for (int t = a.rp[i] + tid; t < a.rp[i + 1]; t += 64) {
                    const int j = a.ci[t];
                    if (j < i) sdot += g.lva[t] * sol[j];
                }
                sdot = wave_sum(sdot);
                if (tid == 0) sol[i] = (r[i] - sdot) / g.ldg[i];
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            for (int i = N - 1; i >= 0; --i) {   // backward with L': row i of L is column i of L'
                const double xi = sol[i] / g.ldg[i];
                __builtin_amdgcn_wave_barrier();
                for (int t = a.rp[i] + tid; t < a.rp[i + 1]; t += 64) {
                    const int j = a.ci[t];
                    if (j < i) sol[j] -= g.lva[t] * xi;
                }
                if (tid == 0) sol[i] = xi;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        for (int i = tid; i < N; i += BT) w[i] = sol[i];
        __syncthreads();
        return;
    }
    // precd 3: p1 = (D + wL) \ r ; p2 = D*p1 ; p = (c*(D + wU)) \ p2
    if (tid < 64) {
        for (int i = 0; i < N; ++i) {   // forward
            double sdot = 0.0;
            for (int t = a.rp[i] + tid; t < a.rp[i + 1]; t += 64) {
                const int j = a.ci[t];
                if (j < i) sdot += a.va[t] * sol[j];
            }
            sdot = wave_sum(sdot);
            if (tid == 0) sol[i] = (r[i] - om * sdot) / dg[i];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        for (int i = tid; i < N; i += 64) sol[i] = dg[i] * sol[i];   // p2
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i = N - 1; i >= 0; --i) {   // backward, in place: rows > i already hold p
            double sdot = 0.0;
            for (int t = a.rp[i] + tid; t < a.rp[i + 1]; t += 64) {
                const int j = a.ci[t];
                if (j > i) sdot += (c * om * a.va[t]) * sol[j];
            }
            sdot = wave_sum(sdot);
            if (tid == 0) sol[i] = (sol[i] - sdot) / (c * dg[i]);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    for (int i = tid; i < N; i += BT) w[i] = sol[i];
    __syncthreads();
    (void)red;
}

__global__ __launch_bounds__(BT) void k_pcg_gen(const PcgGenArgs g) {
    __shared__ double red[16];
    extern __shared__ __attribute__((aligned(16))) double sol[];
    const PcgArgs& a = g.a;
    const int tid = threadIdx.x, N = a.N;
    double* r = a.work;
    double* p = a.work + N;
    double* q = a.work + 2 * (size_t)N;
    double* dg = a.work + 3 * (size_t)N;
    double* w = g.tmp + N;
    // r = e - H*d0 ; diag                                                    PCG.m:68
    for (int row = tid; row < N; row += BT) {
        double sdot = 0.0, dd = 0.0;
        for (int t = a.rp[row]; t < a.rp[row + 1]; ++t) {
            const int j = a.ci[t];
            if (a.guess) sdot += a.va[t] * a.guess[j];
            if (j == row) dd = a.va[t];
        }
        r[row] = a.rhs[row] - sdot;
        dg[row] = dd;
        a.d[row] = a.guess ? a.guess[row] : 0.0;
    }
    __syncthreads();
    if (a.precd == 4) {                                                         // :44-46
        __shared__ int ic_fail;
        if (tid == 0) ic_fail = 0;
        for (int i = tid; i < N; i += BT) sol[i] = 0.0;
        __syncthreads();
        if (tid < 64) pcg_ichol0(g, sol, &ic_fail);
        __syncthreads();
        if (ic_fail) {
            if (tid == 0 && a.out) {
                a.out[0] = -(double)ic_fail;   // nonpositive pivot at row ic_fail - 1
                a.out[1] = NAN;
            }
            return;
        }
    }
    pcg_gen_prec(g, r, w, sol, red);                                            // :69
    double acc = 0.0;
    for (int row = tid; row < N; row += BT) {
        p[row] = w[row];
        acc += r[row] * w[row];
    }
    double delta_new = block_sum(acc, red);
    const double delta_0 = delta_new;
    const double thresh = a.tol * a.tol * delta_0;
    long long it_count = 0;
    while (it_count < a.maxit && delta_new > thresh) {                          // :76
        const double delta_old = delta_new;
        __syncthreads();
        acc = 0.0;
        for (int row = tid; row < N; row += BT) {
            double sdot = 0.0;
            for (int t = a.rp[row]; t < a.rp[row + 1]; ++t) sdot += a.va[t] * p[a.ci[t]];
            q[row] = sdot;
            acc += sdot * p[row];
        }
        const double qp = block_sum(acc, red);
        const double alpha = delta_old / qp;
        for (int row = tid; row < N; row += BT) {
            a.d[row] += alpha * p[row];
            r[row] = r[row] - alpha * q[row];
        }
        __syncthreads();
        pcg_gen_prec(g, r, w, sol, red);                                        // :80
        acc = 0.0;
        for (int row = tid; row < N; row += BT) acc += r[row] * w[row];
        delta_new = block_sum(acc, red);
        const double beta = delta_new / delta_old;
        for (int row = tid; row < N; row += BT) p[row] = w[row] + beta * p[row];
        ++it_count;
        if (tid == 0 && a.out && it_count <= a.nresk)
            a.out[1 + it_count] = sqrt(fabs(delta_new / delta_0));
    }
    if (tid == 0 && a.out) {
        a.out[0] = (double)it_count;
        a.out[1] = sqrt(fabs(delta_new / delta_0));
    }
}

// ---------------------------------------------------------------------------
// fused single-workgroup program
// ---------------------------------------------------------------------------
// Phases whose row range fits one workgroup (a few thousand nonzeros) cost far more as
// launches (2.3 us floor + 3-10 us of latency each, and only 1-8 CUs busy) than as
// work.  The host therefore strings consecutive small phases -- e.g. the ten Gauss-
// Seidel half sweeps, the residual and the restriction of a small fine level, or
// restriction + coarsest PCG + prolongation -- into ONE launch of this kernel: one
// workgroup interprets the descriptor list, with a workgroup barrier between phases.
// Descriptors travel as kernel arguments (no upload, captured by value in graphs).
struct ResidDesc {
    LevelDev lv;
    const double* e;
    int row0, row1;
};
enum : int { PH_SMOOTH = 1, PH_RESID, PH_XFER, PH_TOP, PH_PCG, PH_CONV };
struct PhaseDesc {
    int type;
    int pad_;
    union U {
        SmoothArgs s;
        ResidDesc r;
        XferArgs x;
        TopArgs t;
        PcgArgs p;
        ConvArgs c;
    } u;
};
static constexpr int FUSED_MAX = 16;
struct FusedProg {
    int n;
    int pad_;
    PhaseDesc d[FUSED_MAX];
};
static_assert(sizeof(FusedProg) <= 3900, "fused program must fit the 4 KiB kernel-argument segment");

__global__ __launch_bounds__(BT) void k_fused(FusedProg prog) {
    __shared__ PhaseLds lds;
    __shared__ double red[16];
    extern __shared__ __attribute__((aligned(16))) double xs_dyn[];
    for (int i = 0; i < prog.n; ++i) {
        const PhaseDesc& d = prog.d[i];
        switch (d.type) {
            case PH_SMOOTH:
                if (d.u.s.lv.S > 0)
                    phase_smooth<true, true>(d.u.s, 0, 1, &lds, xs_dyn);
                else
                    phase_smooth<true, false>(d.u.s, 0, 1, &lds, xs_dyn);
                break;
            case PH_RESID:
                if (d.u.r.lv.S > 0)
                    phase_resid<true, true>(d.u.r.lv, d.u.r.e, d.u.r.row0, d.u.r.row1, 0, 1, &lds,
                                            xs_dyn);
                else
                    phase_resid<true, false>(d.u.r.lv, d.u.r.e, d.u.r.row0, d.u.r.row1, 0, 1, &lds,
                                             xs_dyn);
                break;
            case PH_XFER:
                phase_xfer<true>(d.u.x, 0, 1, &lds, xs_dyn);
                break;
            case PH_TOP:
                if (d.u.t.lv.S > 0)
                    phase_top<true, true>(d.u.t, 0, 1, &lds, xs_dyn);
                else
                    phase_top<true, false>(d.u.t, 0, 1, &lds, xs_dyn);
                break;
            case PH_PCG:
                pcg_block(d.u.p, red);
                break;
            case PH_CONV:
                conv_block(d.u.c, red);
                break;
            default:
                break;
        }
        __syncthreads();
    }
}

void pcg_dev(ipd_ctx* ctx, const Csr& H, const double* e, const double* guess, double tol,
             long long maxit, int precd, double* d, long long* it, double* res,
             double* resk_host, long long nf) {
    IPD_REQUIRE(H.nr == H.nc, IPD_E_ARG, "PCG: H must be square");
    IPD_REQUIRE(precd >= 1 && precd <= 5, IPD_E_ARG, "PCG: precd must be 1..5");
    if (precd == 5)
        IPD_REQUIRE(nf > 0 && nf < H.nr, IPD_E_ARG,
                    "SSOR for bigraph requires pcg_options.nf!!!");              // PCG.m:64
    Arena& tmp = *ctx->scratch;
    const long long nresk = resk_host ? std::min<long long>(maxit, 1 << 20) : 0;
    PcgArgs a;
    a.N = H.nr;
    a.L = std::min(pick_lanes(H.nnz, H.nr, 1), PCG_LANES_MAX);
    a.rp = H.rp;
    a.ci = H.ci;
    a.va = H.va;
    a.rhs = e;
    a.guess = guess;
    a.d = d;
    a.work = tmp.alloc<double>(4 * (size_t)H.nr);
    a.tol = tol;
    a.maxit = maxit;
    a.precd = precd;
    a.out = tmp.alloc<double>((size_t)(2 + nresk));
    a.nresk = nresk;
    if (precd == 3 || precd == 4 || precd == 5) {
        IPD_REQUIRE(H.nr <= 7000, IPD_E_LIMIT, "PCG precd 3/4/5: at most 7000 rows (LDS-resident solve)");
        PcgGenArgs g;
        g.a = a;
        g.nf = (int)nf;
        g.tmp = tmp.alloc<double>(2 * (size_t)H.nr);
        g.lva = precd == 4 ? tmp.alloc<double>((size_t)std::max(H.nnz, 1)) : nullptr;
        g.ldg = precd == 4 ? tmp.alloc<double>((size_t)H.nr) : nullptr;
        IPD_OPTIN_LDS(ctx, k_pcg_gen, 60 * 1024);
        hipLaunchKernelGGL(k_pcg_gen, dim3(1), dim3(BT), sizeof(double) * (size_t)H.nr, ctx->stream, g);
    } else {
        hipLaunchKernelGGL(k_pcg, dim3(1), dim3(BT), 0, ctx->stream, a);
    }
    IPD_KERNEL_CHECK();
    if (it || res || resk_host || precd == 4) {
        double head[2];
        ctx->fetch(a.out, head, 2);
        IPD_REQUIRE(!(head[0] < 0.0), IPD_E_NUMERIC,
                    "PCG: ichol encountered a nonpositive pivot (PCG.m:46)");
        if (it) *it = (long long)head[0];
        if (res) *res = head[1];
        if (resk_host && head[0] > 0)
            ctx->fetch(a.out + 2, resk_host, (size_t)std::min<long long>((long long)head[0], nresk));
    }
}

// ---------------------------------------------------------------------------
// matrix-free level-1 operator (the ASAtz.m idea, made to work)
// ---------------------------------------------------------------------------
// In Hybrid_AMG's rescaled system Ae = bk1*Q0^2 + (Q0*T*Q0 + Q0*H0*Q0)/tk the off-diagonal
// block is the active-set mask times a rank-one matrix: Ae(j, n+i) = -s_ij * (q_j^2/tk) * p_i^2.
// A Gauss-Seidel half sweep on the bipartite level therefore needs ONE BIT per entry plus
// two scale vectors instead of 12 bytes: at rho = 1, m = n = 1024 a half sweep reads 128 KB of
// mask instead of 12.6 MB of CSR.  The operator is derived from A_1's own CSR arrays and is
// used only if every entry matches the rank-one form to 1e-12 (k_maskop_build verifies), so a
// caller that hands in any other matrix silently keeps the CSR kernels.
struct MaskOp {
    int nf, nc;           // F rows (column constraints, n), C rows (row constraints, m)
    int nwf, nwc;         // 64-bit words per F row (over i) and per C row (over j)
    const unsigned long long* fbits;  // [nf][nwf]
    const unsigned long long* cbits;  // [nc][nwc]
    const double* alpha;  // nf: q_j^2 / tk
    const double* beta;   // nc: p_i^2
    const double* diag;   // nf + nc
};

// one wave per row: sets the row's bits, checks the rank-one form; bad[0] != 0 on any mismatch
__global__ __launch_bounds__(256) void k_maskop_build(int N, int nf, const int* __restrict__ rp,
                                                      const int* __restrict__ ci,
                                                      const double* __restrict__ va,
                                                      const double* __restrict__ alpha,
                                                      const double* __restrict__ beta, int nwf,
                                                      int nwc, unsigned long long* __restrict__ fbits,
                                                      unsigned long long* __restrict__ cbits,
                                                      double* __restrict__ diag, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    for (int r = wave; r < N; r += nwaves) {
        const bool frow = r < nf;
        bool wrong = false;
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            const int c = ci[t];
            const double v = va[t];
            if (c == r) {
                diag[r] = v;
                continue;
            }
            if (frow == (c < nf)) {   // an entry inside the F or the C block: not bipartite
                wrong = true;
                continue;
            }
            const int j = frow ? r : c, i = (frow ? c : r) - nf;
            const double ref = -(alpha[j] * beta[i]);
            if (!(fabs(v - ref) <= 1e-12 * fabs(ref))) wrong = true;
            if (frow)
                atomicOr(&fbits[(size_t)r * nwf + (i >> 6)], 1ull << (i & 63));
            else
                atomicOr(&cbits[(size_t)(r - nf) * nwc + (j >> 6)], 1ull << (j & 63));
        }
        if (wrong) atomicExch(bad, 1);
    }
}

// One half (F rows or C rows) of the bigraph Gauss-Seidel sweep, same arithmetic as
// phase_smooth (SmoothArgs semantics) with the row sums taken from the bit mask.  A wave owns
// a row; lane l walks 16 bits of word l/4; the operand half vector is staged pre-scaled.
static constexpr int MASK_RW = 1;   // rows per wave of k_smooth_mask

__global__ __launch_bounds__(BT) void k_smooth_mask(const SmoothArgs a, const MaskOp mo) {
    extern __shared__ __attribute__((aligned(16))) double xs[];
    __shared__ double red[16];
    const LevelDev& lv = a.lv;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool frows = a.row0 < mo.nf;          // this launch updates F rows; operands are C columns
    const int oplen = frows ? mo.nc : mo.nf, opoff = frows ? mo.nf : 0;
    const double* __restrict__ scale = frows ? mo.beta : mo.alpha;
    const double* __restrict__ osc = frows ? mo.alpha : mo.beta;   // the row's own scale
    const bool ez = a.eold_zero != 0;
    const bool skip = ez && a.u0 >= a.u1;       // nothing to gather: A*e == 0
    const bool nsp = a.isnsp != 0;
    const int nw = frows ? mo.nwf : mo.nwc;
    // ---- one burst of independent requests: the rows' own scalars, the pieces of
    // xig = 1'r - (A1)'e_old, the operand half vector (pre-scaled, zero-padded to whole words)
    const int RW = min(MASK_RW, 64 / nw);       // rows per wave: their mask words fill <= 64 lanes
    const int row_first =
        __builtin_amdgcn_readfirstlane(a.row0 + (blockIdx.x * (BT / 64) + wv) * RW);
    // the wave's RW*nw mask words are contiguous: lane l fetches word l now, the row loops
    // broadcast them with readlane (fetching them per row cost a global round trip per row)
    unsigned long long wreg = 0;
    {
        const unsigned long long* __restrict__ bits0 = frows ? mo.fbits : mo.cbits;
        const int lr0 = row_first - (frows ? 0 : mo.nf);
        if (!skip && lane < RW * nw && row_first + lane / nw < a.row1)
            wreg = bits0[(size_t)lr0 * nw + lane];
    }
    double eo[MASK_RW], rv[MASK_RW], dv[MASK_RW], axi[MASK_RW], dg[MASK_RW], os[MASK_RW];
#pragma unroll
    for (int u = 0; u < MASK_RW; ++u) {
        const int row = min(row_first + u, a.row1 - 1);
        eo[u] = ez ? 0.0 : a.eold[row];
        rv[u] = lv.r[row];
        dv[u] = lv.dinv[row];
        axi[u] = nsp ? lv.Axi[row] : 0.0;
        dg[u] = mo.diag[row];
        os[u] = osc[row - (frows ? 0 : mo.nf)];
    }
    double cpart = 0.0;
    if (nsp)
        for (int j = tid; j < lv.N; j += BT) cpart += lv.r[j] - lv.Axi[j] * (ez ? 0.0 : a.eold[j]);
    if (!skip)
        for (int t = tid; t < nw * 64; t += BT) {
            const int j = opoff + t;
            double x = 0.0;
            if (t < oplen) x = scale[t] * ((j >= a.u0 && j < a.u1) ? a.win[j] : (ez ? 0.0 : a.eold[j]));
            xs[t] = x;
        }
    double c = 0.0;
    if (nsp) c = block_sum(cpart, red) / lv.xx[0];   // MG_Vcycle.m:19 (block_sum synchronises)
    else __syncthreads();
    const unsigned wlo = (unsigned)wreg, whi = (unsigned)(wreg >> 32);
#pragma unroll
    for (int u = 0; u < MASK_RW; ++u) {
        const int row = row_first + u;
        if (u >= RW || row >= a.row1) break;   // wave-uniform
        double s = 0.0;
        if (!skip) {
            // lane l owns bit l of every word; the operands xs[64*w + l] are conflict-free
            for (int wi = 0; wi < nw; ++wi) {
                const unsigned lo = __builtin_amdgcn_readlane(wlo, u * nw + wi);
                const unsigned hi = __builtin_amdgcn_readlane(whi, u * nw + wi);
                const unsigned half = lane < 32 ? lo : hi;
                const double x = xs[wi * 64 + lane];
                s += ((half >> (lane & 31)) & 1u) ? x : 0.0;
            }
            s = wave_sum(s);
        }
        if (lane == 0) {
            const double ae = dg[u] * eo[u] - os[u] * s;        // (A x)_row
            const double g_i = rv[u] - ae - axi[u] * c;
            const double wvl = eo[u] + dv[u] * g_i;             // e + R*(g - Axi*c)
            if (a.wout) a.wout[row] = wvl;
            a.enew[row] = wvl + c;                              //   ... + xi*c
        }
    }
}

// ---------------------------------------------------------------------------
// whole Class_AMG solve phase in ONE workgroup
// ---------------------------------------------------------------------------
// Realistic Newton systems have tiny hierarchies (every level a few thousand nonzeros,
// SURVEY F4/F5): a W cycle is then several hundred dependent micro-phases and the
// multi-launch path is bound by launch latency and by the host (measured 1.9 ms per
// W cycle at M = 1000).  Here one workgroup interprets the V/W recursion itself
// (MG_Vcycle.m:12-45, MG_Wcycle.m:13-46), the stationary iteration and its stopping
// rules (Class_AMG.m:86-109): one launch and one read-back per solve.
struct SolveLevel {
    LevelDev lv;
    double* e;
    double* e2;
    double* w;
    XferArgs rest;  // r_{k+1} = P' rr_k      (valid for k < J)
    XferArgs prol;  // e_k += P e_{k+1}
    int nnzA, nnzP;  // sizes for the LDS cache copy
    // tiny levels (<= 32 rows) also carry DENSE column-major copies in LDS: M[i + j*rows].
    // Their operators are 50-90 % full, and a dense row walk has affine, independent LDS
    // addresses (no index -> value dependency), which is what a single wave needs to pipeline.
    const double* dA;   // N x N
    const double* dP;   // N x Nc   (prolongation, k < J)
    const double* dPt;  // Nc x N   (restriction,  k < J)
    // One-wave levels in POLYNOMIAL form (k_pack_poly, see tiny_cycle): the nu sweeps of a visit are
    // one fixed linear map, e' = S^nu e + (I + S + ... + S^(nu-1)) Rg r, so the level carries the
    // stacked dense operators below instead of dA / dP / dPt and a visit is two passes.  NULL: sweeps.
    // Layout: column-major with a fixed leading dimension pLD in {32, 48, 64} >= N + Nc and the column
    // count padded to a multiple of 8 with zero columns (the vectors of these levels are zero-padded
    // likewise): every load of a pass then has a compile-time offset from one base address.
    // pMr, pMe, pMc lie one behind the other in the image (a pass streams through them).
    const double* pMr;  // [M2a; P' - (P'A) M2a]  applied to r          (M2 = M2a + w 1': see k_pack_poly)
    const double* pMe;  // [M1; -(P'A) M1]        applied to the iterate (kept start, post-smoothing)
    const double* pMc;  // M1 P                   applied to the child's correction
    const double* pW;   // [w; -(P'A) w]          times 1'r
    int pLD;
    // Thread-per-row levels: lane map (k_pack_lmap, see blk_sweeps) -- BT words {row | sub << 10 |
    // log2(lanes of the row) << 14 | valid << 31} and one word "entries per lane" (0: walk in a loop).
    const unsigned* lmap;
    // Small, nearly full thread-per-row levels (level 4 of the early Newton systems: 60-100 rows, 50-100 %
    // full): the image carries the dense copy dA instead of the CSR arrays, and a lane keeps its part of
    // the row (columns sub, sub + Lr, ...) in registers for the visit (blk_sweeps).
    int blk_dense;
    // Thread-per-row levels of 49..144 rows in BLOCK-WIDE polynomial form (k_bpoly_*, see bpoly_pass):
    // the same stacked operators as pMr / pMe / pMc, [Mr | Me | Mc] one behind the other, column-major
    // with gLD in {128, 256} rows, in GLOBAL memory (they do not fit in LDS: 200-500 KB; the tail's
    // compute unit streams them from L2 twice per visit).  NULL: sweeps.
    const double* gM;
    const double* gW;
    int gLD;
};
struct SolveDesc {
    int J, nu, isnsp, wcycle, anycycle, maxit;
    int k_lds;        // levels k_lds..J (and the transfers between them) are cached in LDS
    int k_tiny;       // levels k_tiny..J have <= 32 rows: their whole sub-cycle runs in ONE wave
    int k_blk;        // cached Jacobi levels k_blk..k_tiny-1: one thread per row (blk_cycle)
    int k_semi;       // 0, or a sub-cycle root whose vectors sit in LDS while its matrix, its
                      // transfers and its constant vectors are read from global memory (L2)
    // LDS image: this descriptor, a relocation table and the constant arrays of the cached
    // levels are laid out in global memory exactly as they will sit in LDS (behind the staging
    // area); pointers into the image are stored as LDS byte offsets and relocated on arrival
    int image_bytes;  // multiple of 16; 0 = nothing cached
    int lds_total;    // dynamic LDS the kernel is launched with: staging area, image, work vectors
    int dbg_skip;     // timing by elimination (IPD_DEBUG_SKIP=<mask>, results are then garbage): 1 the
                      // polynomial passes skip their streams, 2 the coarsest PCG does no iteration, 4 the
                      // thread-per-row sweeps skip the row walk, 8 no sweeps at all on those levels
    int nreloc;
    double* root_r;   // k_subcycle: global right-hand side / correction of the root level
    double* root_e;
    long long* dbg;   // optional: wall_clock64 stamps (100 MHz) of k_subcycle's stages
    int stage_bytes;  // size of the gather staging area at the start of dynamic LDS
    double* bp_part;  // LDS: 8 x gLD partial sums + 8 (block-wide polynomial passes)
    // One block-wide polynomial level's operator as an LDS copy (round 4): a compact column-major copy of
    // L[bm_level].gM with bm_ld rows (the stacked N + Nc <= 128, rounded up to even) sits at bm_src; a kernel whose
    // launch carries lds_total + bm_bytes of dynamic LDS (the resident kernels' tail workgroup, which serves a whole
    // solve out of one image load) copies it to LDS offset bm_off and its passes read it there -- 0.7 us per pass
    // against 1.7 us out of L2.  bm_bytes = 0: none.
    const double* bm_src;
    int bm_level, bm_ld, bm_off, bm_bytes;
    double retol;
    PcgArgs pcg;
    SolveLevel L[SOLVE_ML + 1];
};

struct SolveCtx {  // per-thread copies of uniform state
    const SolveDesc* D;
    PhaseLds* lds;
    double* red;
    double* xs;
    unsigned swapmask;  // bit k: the current iterate of level k lives in e2
    unsigned zeromask;  // bit k: the iterate of level k is identically zero (not materialised)
    double* part;       // 3 x 16 per-wave partial sums (blk_cycle)
    double* sumr;       // per-level sum of the right-hand side (blk_cycle)
    long long* dbg;     // optional stage clocks (ipd_amg_bench_subcycle), NULL in production
    unsigned bm_lds;    // LDS address of the loaded operator copy (SolveDesc::bm_src), 0: not loaded
};
// accumulates the 100 MHz clock spent since t0 into dbg[slot] (thread 0 only)
#define SOL_DBG_T0(c) const long long dbg_t0__ = (c).dbg ? wall_clock64() : 0
#define SOL_DBG_ADD(c, slot)                                                     \
    do {                                                                         \
        if ((c).dbg && threadIdx.x == 0) (c).dbg[slot] += wall_clock64() - dbg_t0__; \
    } while (0)

__device__ __forceinline__ double* sol_e(const SolveCtx& c, int k) {
    return ((c.swapmask >> k) & 1u) ? c.D->L[k].e2 : c.D->L[k].e;
}
__device__ __forceinline__ double* sol_e2(const SolveCtx& c, int k) {
    return ((c.swapmask >> k) & 1u) ? c.D->L[k].e : c.D->L[k].e2;
}

__device__ __forceinline__ void sol_smooth_call(SolveCtx& c, const SmoothArgs& a) {
    phase_smooth<true, false>(a, 0, 1, c.lds, c.xs);  // descriptors carry S = 0: CSR walk only
    __syncthreads();
}

__device__ __forceinline__ void sol_sweep(SolveCtx& c, int k, bool post) {
    const SolveLevel& L = c.D->L[k];
    SmoothArgs a;
    a.lv = L.lv;
    a.eold = sol_e(c, k);
    a.enew = sol_e2(c, k);
    a.win = L.w;
    a.wout = L.w;
    a.isnsp = c.D->isnsp;
    a.staged = 1;
    a.eold_zero = (c.zeromask >> k) & 1u;
    const int nf = L.lv.nf, N = L.lv.N;
    if (nf == 0) {
        a.row0 = 0;
        a.row1 = N;
        a.u0 = a.u1 = 0;
        a.wout = nullptr;
        sol_smooth_call(c, a);
    } else {
        const int f0 = post ? nf : 0, f1 = post ? N : nf;
        const int s0 = post ? 0 : nf, s1 = post ? nf : N;
        a.row0 = f0;
        a.row1 = f1;
        a.u0 = a.u1 = 0;
        sol_smooth_call(c, a);
        a.row0 = s0;
        a.row1 = s1;
        a.u0 = f0;
        a.u1 = f1;
        a.wout = nullptr;
        sol_smooth_call(c, a);
    }
    c.swapmask ^= (1u << k);
    c.zeromask &= ~(1u << k);
}

// ---- LDS-resident sub-cycles ---------------------------------------------------------------
// Everything below works on levels whose matrices and vectors sit in LDS.  The descriptor
// keeps GENERIC pointers (the same struct also describes global levels), and a load through
// a generic pointer is a FLAT instruction: it takes the vector-memory path and several
// hundred cycles even when it lands in LDS (measured: 2.3 us for a 6-entries-per-row sweep).
// So each visit first copies what it needs into registers as address_space(3) pointers;
// the row walks then compile to ds_read.
#define AS3 __attribute__((address_space(3)))
// (the low 32 bits of a generic pointer into the LDS aperture ARE its LDS address; a plain
// addrspacecast adds a null test per pointer, ~100 VALU instructions per lds_level() call)
template <class T>
__device__ __forceinline__ AS3 T* as_lds(T* p) {
    return (AS3 T*)(unsigned)(size_t)p;
}

struct LdsLevel {
    int N, Nc;
    AS3 const int* rp;
    AS3 const int* ci;
    AS3 const double* va;
    AS3 const double* dinv;
    AS3 const double* Axi;
    AS3 double* r;
    AS3 double* rr;
    AS3 double* e;    // current iterate (swap parity applied)
    AS3 double* e2;
    AS3 double* rc;   // child's right-hand side
    AS3 const int* Rrp;   // restriction P' (CSR, Nc rows)
    AS3 const int* Rci;
    AS3 const double* Rva;
    AS3 const int* Prp;   // prolongation P (CSR, N rows)
    AS3 const int* Pci;
    AS3 const double* Pva;
    AS3 const double* dA;   // dense copies (tiny levels only)
    AS3 const double* dP;
    AS3 const double* dPt;
    AS3 const double* pMr;  // polynomial form (tiny levels, see SolveLevel); NULL: sweeps
    AS3 const double* pMe;
    AS3 const double* pMc;
    AS3 const double* pW;
    int pLD;
    bool poly;
    AS3 const double* bM;   // LDS copy of gM (SolveDesc::bm_src), NULL: read gM from global memory
    AS3 const double* bW;   // ... and of gW behind it
    int bLD;
    AS3 const unsigned* lmap;
    bool mapped;
    bool bdense;
    const double* gM;   // block-wide polynomial form (global memory); NULL: sweeps
    const double* gW;
    int gLD;
    double xx;
    // semi-cached level: a 1024-row level does not fit in LDS beside the deeper ones, but its
    // rows are short (3-7 entries) and L2-resident; only r, e, e2 live in LDS
    bool semi;
    const int* grp;
    const int* gci;
    const double* gva;
    const double* gdinv;
    const double* gAxi;
    const int* gRrp;
    const int* gRci;
    const double* gRva;
    const int* gPrp;
    const int* gPci;
    const double* gPva;
};
__device__ __forceinline__ double lvl_dinv(const LdsLevel& L, int i) { return L.semi ? L.gdinv[i] : L.dinv[i]; }
__device__ __forceinline__ double lvl_axi(const LdsLevel& L, int i) { return L.semi ? L.gAxi[i] : L.Axi[i]; }

__device__ __forceinline__ LdsLevel lds_level(const SolveCtx& c, int k) {
    const AS3 SolveDesc* D = (const AS3 SolveDesc*)c.D;
    const AS3 SolveLevel& G = D->L[k];
    LdsLevel L;
    L.N = G.lv.N;
    L.Nc = G.rest.nrows;
    L.rp = as_lds(G.lv.rp);
    L.ci = as_lds(G.lv.ci);
    L.va = as_lds(G.lv.va);
    L.dinv = as_lds(G.lv.dinv);
    L.Axi = as_lds(G.lv.Axi);
    L.r = as_lds(G.lv.r);
    L.rr = as_lds(G.lv.rr);
    const bool sw = (c.swapmask >> k) & 1u;
    L.e = as_lds(sw ? G.e2 : G.e);
    L.e2 = as_lds(sw ? G.e : G.e2);
    L.rc = as_lds(G.rest.y);
    L.Rrp = as_lds(G.rest.rp);
    L.Rci = as_lds(G.rest.ci);
    L.Rva = as_lds(G.rest.va);
    L.Prp = as_lds(G.prol.rp);
    L.Pci = as_lds(G.prol.ci);
    L.Pva = as_lds(G.prol.va);
    L.dA = as_lds(G.dA);
    L.dP = as_lds(G.dP);
    L.dPt = as_lds(G.dPt);
    L.pMr = as_lds(G.pMr);
    L.pMe = as_lds(G.pMe);
    L.pMc = as_lds(G.pMc);
    L.pW = as_lds(G.pW);
    L.pLD = G.pLD;
    L.poly = G.pMr != nullptr;
    L.lmap = as_lds(G.lmap);
    L.mapped = G.lmap != nullptr;
    L.bdense = G.blk_dense != 0;
    L.gM = G.gM;
    L.gW = G.gW;
    L.gLD = G.gLD;
    L.bM = (c.bm_lds && D->bm_level == k) ? (AS3 const double*)c.bm_lds : (AS3 const double*)0;
    L.bLD = D->bm_ld;
    L.bW = L.bM + (D->bm_bytes / 8 - D->bm_ld);
    L.semi = (k == D->k_semi);
    L.grp = G.lv.rp;
    L.gci = G.lv.ci;
    L.gva = G.lv.va;
    L.gdinv = G.lv.dinv;
    L.gAxi = G.lv.Axi;
    L.gRrp = G.rest.rp;
    L.gRci = G.rest.ci;
    L.gRva = G.rest.va;
    L.gPrp = G.prol.rp;
    L.gPci = G.prol.ci;
    L.gPva = G.prol.va;
    L.xx = L.semi ? G.lv.xx[0] : as_lds(G.lv.xx)[0];
    return L;
}
__device__ __forceinline__ AS3 double* lds_e(const SolveCtx& c, int k) {
    const AS3 SolveDesc* D = (const AS3 SolveDesc*)c.D;
    return as_lds(((c.swapmask >> k) & 1u) ? D->L[k].e2 : D->L[k].e);
}

// A wave is its own barrier: LDS operations of one wave execute in order; the fence only
// stops the compiler from reordering them.
__device__ __forceinline__ void tiny_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// sparse row walk, four entries per step: the index loads, then the gathers, are independent,
// so the LDS latency is paid once per step instead of once per entry; the sum keeps its order
__device__ __forceinline__ double lds_rowdot(AS3 const int* rp, AS3 const int* ci,
                                             AS3 const double* va, int row, bool valid,
                                             AS3 const double* x) {
    double s = 0.0;
    if (valid) {
        int t = rp[row];
        const int end = rp[row + 1];
        for (; t + 4 <= end; t += 4) {
            const int c0 = ci[t], c1 = ci[t + 1], c2 = ci[t + 2], c3 = ci[t + 3];
            const double v0 = va[t], v1 = va[t + 1], v2 = va[t + 2], v3 = va[t + 3];
            const double x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
            s += v0 * x0;
            s += v1 * x1;
            s += v2 * x2;
            s += v3 * x3;
        }
        for (; t < end; ++t) s += va[t] * x[ci[t]];
    }
    return s;
}

// The coarse levels have a few long rows (hubs: 60+ entries against a mean of 6), and with one
// thread per row the whole block waits for them at every barrier (measured: 70 % of a sweep).
// So a row is walked by Lr consecutive lanes (Lr = largest power of two with rows*Lr <= 1024,
// at most 16), entries strided over the lanes, partial sums combined with DPP row operations.
#ifndef IPD_BLK_LANES
#define IPD_BLK_LANES BT
#endif
__device__ __forceinline__ int lanes_per_row(int rows) {
    int L = 1;
    while (L < 16 && rows * (L * 2) <= IPD_BLK_LANES) L <<= 1;
    return L;
}
// every lane of the group returns the full sum.  Entries go four at a time with the last batch
// masked instead of a one-by-one remainder loop: most rows of these levels hold fewer than
// 4*Lr entries, and the remainder loop paid two dependent LDS round trips per entry.
#ifndef IPD_LDS_ROW_U
#define IPD_LDS_ROW_U 2
#endif
static constexpr int LDS_ROW_U = IPD_LDS_ROW_U;   // entries per lane and trip of the LDS row walk
// (entry range given: the sweeps of a visit read a row's pointers once, not once per sweep)
template <int U = LDS_ROW_U>
__device__ __forceinline__ double lds_rowdot_range(AS3 const int* ci, AS3 const double* va, int beg,
                                                   int end, int sub, int Lr, AS3 const double* x) {
    constexpr int LDS_ROW_U = U;
    double s = 0.0;
    for (int t = beg + sub; t < end; t += LDS_ROW_U * Lr) {
        int c[LDS_ROW_U];
        double v[LDS_ROW_U], xv[LDS_ROW_U];
        bool k[LDS_ROW_U];
#pragma unroll
        for (int u = 0; u < LDS_ROW_U; ++u) {
            const int tu = t + u * Lr;
            k[u] = tu < end;
            c[u] = ci[k[u] ? tu : t];
            v[u] = va[k[u] ? tu : t];
        }
#pragma unroll
        for (int u = 0; u < LDS_ROW_U; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < LDS_ROW_U; ++u)
            if (k[u]) s += v[u] * xv[u];
    }
    return subwave_sum(s, Lr);
}
__device__ __forceinline__ double lds_rowdot_split(AS3 const int* rp, AS3 const int* ci,
                                                   AS3 const double* va, int row, int sub, int Lr,
                                                   bool valid, AS3 const double* x) {
    double s = 0.0;
    if (valid) {
        const int beg = rp[row], end = rp[row + 1];
        for (int t = beg + sub; t < end; t += LDS_ROW_U * Lr) {
            int c[LDS_ROW_U];
            double v[LDS_ROW_U], xv[LDS_ROW_U];
            bool k[LDS_ROW_U];
#pragma unroll
            for (int u = 0; u < LDS_ROW_U; ++u) {
                const int tu = t + u * Lr;
                k[u] = tu < end;
                c[u] = ci[k[u] ? tu : t];
                v[u] = va[k[u] ? tu : t];
            }
#pragma unroll
            for (int u = 0; u < LDS_ROW_U; ++u) xv[u] = x[c[u]];
#pragma unroll
            for (int u = 0; u < LDS_ROW_U; ++u)
                if (k[u]) s += v[u] * xv[u];
        }
    }
    return subwave_sum(s, Lr);
}

// the same walk with the matrix in global memory (semi-cached level); x is in LDS
__device__ __forceinline__ double glb_rowdot_split(const int* __restrict__ rp,
                                                   const int* __restrict__ ci,
                                                   const double* __restrict__ va, int row, int sub,
                                                   int Lr, bool valid, AS3 const double* x) {
    double s = 0.0;
    if (valid) {
        const int beg = rp[row], end = rp[row + 1];
        for (int t = beg + sub; t < end; t += 4 * Lr) {
            const int t1 = t + Lr, t2 = t + 2 * Lr, t3 = t + 3 * Lr;
            const bool k1 = t1 < end, k2 = t2 < end, k3 = t3 < end;
            const int c0 = ci[t], c1 = ci[k1 ? t1 : t], c2 = ci[k2 ? t2 : t], c3 = ci[k3 ? t3 : t];
            const double v0 = va[t], v1 = va[k1 ? t1 : t], v2 = va[k2 ? t2 : t], v3 = va[k3 ? t3 : t];
            s += v0 * x[c0];
            if (k1) s += v1 * x[c1];
            if (k2) s += v2 * x[c2];
            if (k3) s += v3 * x[c3];
        }
    }
    return subwave_sum(s, Lr);
}
// Semi-cached level with LONG rows (a level 3 of a few hundred rows with 40-100 entries each, too big
// for LDS beside the deeper levels): Lr lanes per row, eight entries per lane and trip in flight
// (a trip is a round trip to L2), the row's entry range read once per visit.
__device__ __forceinline__ double glb_rowdot_range(const int* __restrict__ ci, const double* __restrict__ va,
                                                   int beg, int end, int sub, int Lr, AS3 const double* x) {
    constexpr int U = 8;
    double s = 0.0;
    for (int t = beg + sub; t < end; t += U * Lr) {
        int c[U];
        double v[U];
        bool k[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int tu = t + u * Lr;
            k[u] = tu < end;
            c[u] = ci[k[u] ? tu : t];
            v[u] = va[k[u] ? tu : t];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k[u]) s += v[u] * x[c[u]];
    }
    return subwave_sum(s, Lr);
}
// A semi-cached level walks its rows thread-per-row; the first SEMI_RC entries of the row stay in
// registers for all sweeps of a visit (a global round trip per sweep would cost more than the
// launch the kernel replaces), longer rows read the rest from global memory.
static constexpr int SEMI_RC = 6;
struct SemiRow {
    int c[SEMI_RC];
    double v[SEMI_RC];
    int t0, len;
};
__device__ __forceinline__ SemiRow semi_row_load(const LdsLevel& L, int row, bool valid) {
    SemiRow R;
    R.t0 = valid ? L.grp[row] : 0;
    R.len = valid ? L.grp[row + 1] - R.t0 : 0;
#pragma unroll
    for (int u = 0; u < SEMI_RC; ++u) {
        const bool in = u < R.len;
        R.c[u] = in ? L.gci[R.t0 + u] : 0;
        R.v[u] = in ? L.gva[R.t0 + u] : 0.0;
    }
    return R;
}
__device__ __forceinline__ double semi_row_dot(const LdsLevel& L, const SemiRow& R,
                                               AS3 const double* x) {
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < SEMI_RC; ++u) {
        const double term = R.v[u] * x[R.c[u]];
        s = (u < R.len) ? s + term : s;
    }
    for (int t = R.t0 + SEMI_RC; t < R.t0 + R.len; ++t) s += L.gva[t] * x[L.gci[t]];
    return s;
}

// y_i = sum_j M[i + j*rows] * x[j]: ascending j like the sorted CSR walk, and the explicit
// zeros add +0.0, so the result has the same bits
__device__ __forceinline__ double lds_densedot(AS3 const double* M, int rows, int cols, int i,
                                               bool valid, AS3 const double* x) {
    double s = 0.0;
    AS3 const double* col = M + (valid ? i : 0);
#pragma unroll 8
    for (int j = 0; j < cols; ++j) s += col[j * rows] * x[j];
    return valid ? s : 0.0;
}

// ---- wave-level sub-cycle: levels with <= 32 rows ----------------------------------------
// A W cycle visits level k 2^(k-1) times, so most of its phases run on the deepest,
// tiniest levels (a dozen rows).  There a 1024-thread phase is all fixed cost (barriers,
// descriptor reads), so ONE wave runs the whole sub-cycle below level k_tiny: lane i owns
// row i, vectors and dense operators live in LDS.  (Keeping the vectors in registers and
// broadcasting with v_readlane was measured 15 % slower: one wave issues an instruction
// every ~5 cycles, and two readlanes per column cost more issue slots than one ds_read.)
// rows are walked by Lt = 2..8 lanes each when the level leaves lanes idle (N <= 32)
__device__ __forceinline__ int tiny_lanes(int rows) {
    int L = 1;
    while (L < 8 && rows * (L * 2) <= 64) L <<= 1;
    return L;
}
// every lane of the row's group returns the full sum (columns strided over the group)
__device__ __forceinline__ double lds_densedot_split(AS3 const double* M, int rows, int cols,
                                                     int row, int sub, int Lt, bool valid,
                                                     AS3 const double* x) {
    double s = 0.0;
    AS3 const double* base = M + (valid ? row : 0);
    int j = sub;
    for (; j + 3 * Lt < cols; j += 4 * Lt) {
        const double a0 = base[j * rows], a1 = base[(j + Lt) * rows], a2 = base[(j + 2 * Lt) * rows],
                     a3 = base[(j + 3 * Lt) * rows];
        const double x0 = x[j], x1 = x[j + Lt], x2 = x[j + 2 * Lt], x3 = x[j + 3 * Lt];
        s += a0 * x0;
        s += a1 * x1;
        s += a2 * x2;
        s += a3 * x3;
    }
    for (; j < cols; j += Lt) s += base[j * rows] * x[j];
    s = subwave_sum(s, Lt);
    return valid ? s : 0.0;
}

__device__ __forceinline__ void tiny_sweeps(SolveCtx& c, int k, LdsLevel& L, int nu, int isnsp) {
    const int N = L.N, Lt = tiny_lanes(N);
    const int i = threadIdx.x / Lt, sub = threadIdx.x % Lt;
    const bool valid = i < N, owner = valid && sub == 0;
    const double rv = valid ? L.r[i] : 0.0;
    const double ax = valid ? L.Axi[i] : 0.0;
    const double dv = valid ? L.dinv[i] : 0.0;
    for (int s = 0; s < nu; ++s) {
        const bool ez = (c.zeromask >> k) & 1u;
        const double eo = (valid && !ez) ? L.e[i] : 0.0;
        double cc = 0.0;
        if (isnsp) cc = wave_sum(owner ? rv - ax * eo : 0.0) / L.xx;
        const double sd = ez ? 0.0 : lds_densedot_split(L.dA, N, N, i, sub, Lt, valid, L.e);
        if (owner) L.e2[i] = eo + dv * (rv - sd - ax * cc) + cc;
        tiny_sync();
        AS3 double* t = L.e;
        L.e = L.e2;
        L.e2 = t;
        c.swapmask ^= (1u << k);
        c.zeromask &= ~(1u << k);
    }
}

// ---- polynomial form of a one-wave level --------------------------------------------------
// nu smoothing sweeps are nu applications of ONE affine map, e <- S e + Rg r with
// Rg g = 1 (1'g / xx) + R (g - A1 (1'g) / xx)  (isnsp; MG_Vcycle.m:15-21) or R g, R = Rk{k} = 0.5 D^-1
// (Class_AMG.m:84), S = I - Rg A.  So the sweeps of a visit are e' = M1 e + M2 r with M1 = S^nu,
// M2 = (I + S + ... + S^(nu-1)) Rg: dense N x N matrices (N <= 48) that k_pack_poly forms once per
// hierarchy.  Residual and restriction of the visit (MG_Vcycle.m:27) fold in as well,
//   r_c = P'(r - A e_pre) = (P' - (P'A) M2) r - (P'A) M1 e ,
// and so does the prolongation (MG_Vcycle.m:31) into the post-smoothing,
//   e'' = M1 (e_pre + P e_c) + M2 r = M1 e_pre + (M1 P) e_c + M2 r :
// a visit is TWO passes of independent dense row dots by one wave (~0.3 us each) instead of 2 nu
// dependent sweeps + residual + restriction + prolongation (~9 us at nu = 5).  Same linear operator,
// different rounding (1e-15 relative): the solve phase is compared through residual histories.
// One pass = one stream of 8-column blocks over the operators [Mr | Me | Mc], which lie one behind the
// other in the image (block q of the stream starts at M + q*8*LD), against the vectors x0 (blocks
// [0, n0)), x1 ([n0, n0+n1)), x2 (the rest).  Every load of a block sits at a compile-time offset from
// the block's two base addresses, and the loads of the NEXT block are issued before the current one
// is consumed: with the latency of every trip exposed a pass took 1.0-1.7 us (measured), it is
// bound by LDS issue otherwise.  sx (optional): sum of the entries of x0.
template <int LD>
struct PolyBlk {
    double a[8], v[8];
    __device__ __forceinline__ void load(AS3 const double* pm, AS3 const double* px) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a[u] = pm[u * LD];
            v[u] = px[u];
        }
    }
    __device__ __forceinline__ void use(double (&s)[4], double& sx, double fx) const {
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u & 3] = __builtin_fma(a[u], v[u], s[u & 3]);
        if (fx != 0.0) {   // (uniform per block of a lane's stream)
#pragma unroll
            for (int u = 0; u < 8; ++u) sx += v[u];
        }
    }
};
// (a plain function of scalars: a lambda's closure object ended up in scratch memory, one
// scratch_load per block, because the select between its fields became a load through a selected address)
__device__ __forceinline__ AS3 const double* poly_px(int q, int n0, int n01, unsigned a0, unsigned a1,
                                                     unsigned a2) {
    unsigned base = a2;
    if (q < n01) base = a1;
    if (q < n0) base = a0;
    return (AS3 const double*)(size_t)(base + 64u * (unsigned)q);
}
template <int LD>
__device__ __forceinline__ double poly_stream(AS3 const double* M, int nb, int sub, int Lt, AS3 const double* x0,
                                              int n0, AS3 const double* x1, int n1, AS3 const double* x2,
                                              bool want_sx, double& sx) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    PolyBlk<LD> A, B;
    if (nb <= 0) return 0.0;
    if (Lt == 1) {
        // One lane per row (more than 32 rows: the usual case): the block index is uniform, so the
        // segment selects are scalar and the prefetch is unconditional (the last trip re-reads its own
        // block) -- a load inside a divergent branch makes the compiler wait for ALL outstanding loads
        // at the join (seen in the ISA: s_waitcnt lgkmcnt(0) right behind the prefetch).
        // (the vectors' LDS addresses as plain integers in SGPRs: selecting among the three POINTERS
        // made the compiler park them in scratch memory and fetch the chosen one per block)
        const unsigned a0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)x0);
        const unsigned a1 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)x1) - 64u * (unsigned)n0;
        const unsigned a2 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)x2) - 64u * (unsigned)(n0 + n1);
#define px_of(q) poly_px((q), n0, n0 + n1, a0, a1, a2)
        int q = 0;
        A.load(M, px_of(0));
        for (;;) {
            int qn = q + 1;
            int ql = qn < nb ? qn : q;
            B.load(M + ql * (8 * LD), px_of(ql));
            A.use(s, sx, (want_sx && q < n0) ? 1.0 : 0.0);
            if (qn >= nb) break;
            q = qn;
            qn = q + 1;
            ql = qn < nb ? qn : q;
            A.load(M + ql * (8 * LD), px_of(ql));
            B.use(s, sx, (want_sx && q < n0) ? 1.0 : 0.0);
            if (qn >= nb) break;
            q = qn;
        }
#undef px_of
        return (s[0] + s[1]) + (s[2] + s[3]);
    }
    // several lanes per row (at most 32 rows): each lane walks its own blocks sub, sub + Lt, ...
    for (int q = sub; q < nb; q += Lt) {
        AS3 const double* px = q < n0 ? x0 + 8 * q : (q < n0 + n1 ? x1 + 8 * (q - n0) : x2 + 8 * (q - n0 - n1));
        A.load(M + q * (8 * LD), px);
        A.use(s, sx, (want_sx && q < n0) ? 1.0 : 0.0);
    }
    return (s[0] + s[1]) + (s[2] + s[3]);
}
__device__ __forceinline__ int poly_lanes(int rows) {
    int L = 1;
    while (L < 8 && rows * (L * 2) <= 64) L <<= 1;
    return L;
}
// pre-smoothing + residual + restriction: e2 <- M1 e + M2 r, child's r <- (...) r - (...) e
template <int LD>
__device__ __forceinline__ void poly_pre_ld(SolveCtx& c, int k, LdsLevel& L, bool keep) {
    const int N = L.N, R = L.N + L.Nc, Lt = poly_lanes(R), t = threadIdx.x;
    const int sub = t % Lt, row = t / Lt, rw = row < R ? row : 0, nblk = (N + 7) >> 3;
    double sx = 0.0;
    const int skip = (((const AS3 SolveDesc*)c.D)->dbg_skip & 1) ? 0 : 1;
    double y = poly_stream<LD>(L.pMr + rw, skip * (keep ? 2 * nblk : nblk), sub, Lt, L.r, nblk, L.e, nblk, L.e, true, sx);
    y = subwave_sum(y, Lt);
    sx = subwave_sum(sx, Lt);
    y = __builtin_fma(L.pW[rw], sx, y);
    if (t == 0) as_lds(c.sumr)[k] = sx;      // 1'r of this visit: the post-smoothing pass needs it again
    if (row < R && sub == 0) {
        if (row < N)
            L.e2[row] = y;
        else
            L.rc[row - N] = y;
    }
    tiny_sync();
    AS3 double* tt = L.e;
    L.e = L.e2;
    L.e2 = tt;
    c.swapmask ^= (1u << k);
    c.zeromask &= ~(1u << k);
}
// prolongation + post-smoothing: e2 <- M1 e + (M1 P) e_c + M2 r
template <int LD>
__device__ __forceinline__ void poly_post_ld(SolveCtx& c, int k, LdsLevel& L, AS3 const double* ec) {
    const int N = L.N, Lt = poly_lanes(N), t = threadIdx.x;
    const int sub = t % Lt, row = t / Lt, rw = row < N ? row : 0, nblk = (N + 7) >> 3;
    double dum = 0.0;
    const int skip = (((const AS3 SolveDesc*)c.D)->dbg_skip & 1) ? 0 : 1;
    double y = poly_stream<LD>(L.pMr + rw, skip * (2 * nblk + ((L.Nc + 7) >> 3)), sub, Lt, L.r, nblk, L.e, nblk, ec, false, dum);
    y = subwave_sum(y, Lt);
    y = __builtin_fma(L.pW[rw], as_lds(c.sumr)[k], y);
    if (row < N && sub == 0) L.e2[row] = y;
    tiny_sync();
    AS3 double* tt = L.e;
    L.e = L.e2;
    L.e2 = tt;
    c.swapmask ^= (1u << k);
}
__device__ __forceinline__ void poly_pre(SolveCtx& c, int k, LdsLevel& L, bool keep) {
    if (L.pLD == 32)
        poly_pre_ld<32>(c, k, L, keep);
    else if (L.pLD == 48)
        poly_pre_ld<48>(c, k, L, keep);
    else
        poly_pre_ld<64>(c, k, L, keep);
}
__device__ __forceinline__ void poly_post(SolveCtx& c, int k, LdsLevel& L, AS3 const double* ec) {
    if (L.pLD == 32)
        poly_post_ld<32>(c, k, L, ec);
    else if (L.pLD == 48)
        poly_post_ld<48>(c, k, L, ec);
    else
        poly_post_ld<64>(c, k, L, ec);
}

// PCG.m:68-87 on at most 16 rows (the coarsest level of every realistic hierarchy: thr = 1 + fix(M^(1/3))
// <= 16 up to M = 4096, Class_AMG.m:76).  Row i lives on lane i of the first DPP row, its matrix row in
// registers: the two sums of an iteration are 4-step row sums whose result every lane holds (no
// read-back through an SGPR), the matrix-vector product is one trip of independent LDS reads, the
// reciprocal of delta_old is formed beside that trip, and M^-1 r multiplies by the stored reciprocal
// diagonal.  Measured on 7 / 11 rows: 3.2 / 2.9 -> see DESIGN us per solve.  Same recurrences as
// tiny_pcg; beta and M^-1 r differ from a true division by one rounding.
// 1 / x to full double precision without the division's scaling and fix-up steps (the operands here are
// sums of squares of ordinary magnitude): v_rcp_f64 is good to ~26 bits, two Newton steps take it to 53.
__device__ __forceinline__ double pcg_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = __builtin_fma(__builtin_fma(-x, y, 1.0), y, y);
    y = __builtin_fma(__builtin_fma(-x, y, 1.0), y, y);
    return y;
}
__device__ __forceinline__ void tiny_pcg16(SolveCtx& c, int k, const LdsLevel& L) {
    const AS3 SolveDesc* D = (const AS3 SolveDesc*)c.D;
    const double tol = D->pcg.tol;
    const long long maxit = (D->dbg_skip & 2) ? 0 : D->pcg.maxit;
    const int precd = D->pcg.precd;
    AS3 double* pv = as_lds(D->pcg.work);
    const int N = L.N, i = threadIdx.x;
    const bool valid = i < N;
    const int ir = valid ? i : 0;
    double a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = (valid && j < N) ? L.dA[ir + (j < N ? j : 0) * N] : 0.0;
    const double dg = valid ? L.dA[ir + ir * N] : 1.0;
    const double idg = precd == 2 ? 1.0 / dg : 1.0;
    double r = valid ? L.r[ir] : 0.0;
    double p = precd == 2 ? r / dg : r;
    double d = 0.0;
    double delta_new = row16_sum(r * p);
    delta_new = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(delta_new)),
                                 __builtin_amdgcn_readfirstlane(__double2loint(delta_new)));
    const double thresh = tol * tol * delta_new;
    long long it = 0;
    while (it < maxit && delta_new > thresh) {   // (wave-uniform: delta_new is lane 0's)
        const double delta_old = delta_new;
        if (valid) pv[i] = p;
        tiny_sync();
        const double rcp_old = pcg_rcp(delta_old);
        double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
            if (j >= N) break;   // uniform: whole 4-column chunks only
            const double x0 = pv[j < N ? j : 0], x1 = pv[j + 1 < N ? j + 1 : 0];
            const double x2 = pv[j + 2 < N ? j + 2 : 0], x3 = pv[j + 3 < N ? j + 3 : 0];
            q0 += a[j] * (j < N ? x0 : 0.0);
            q1 += a[j + 1] * (j + 1 < N ? x1 : 0.0);
            q2 += a[j + 2] * (j + 2 < N ? x2 : 0.0);
            q3 += a[j + 3] * (j + 3 < N ? x3 : 0.0);
        }
        const double q = (q0 + q1) + (q2 + q3);
        tiny_sync();
        const double alpha = delta_old * pcg_rcp(row16_sum(q * p));
        d += alpha * p;
        r -= alpha * q;
        const double w = r * idg;
        delta_new = row16_sum(r * w);
        delta_new = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(delta_new)),
                                     __builtin_amdgcn_readfirstlane(__double2loint(delta_new)));
        p = w + (delta_new * rcp_old) * p;
        ++it;
    }
    if (valid) L.e[i] = d;
    tiny_sync();
    c.zeromask &= ~(1u << k);
}

__device__ __forceinline__ void tiny_pcg(SolveCtx& c, int k) {  // PCG.m:68-87, Jacobi, zero guess
    const LdsLevel L = lds_level(c, k);
    if (L.N <= 16) {
        tiny_pcg16(c, k, L);
        return;
    }
    const AS3 SolveDesc* D = (const AS3 SolveDesc*)c.D;
    const double tol = D->pcg.tol;
    const long long maxit = D->pcg.maxit;
    const int precd = D->pcg.precd;
    AS3 double* pv = as_lds(D->pcg.work);  // p shared through LDS
    const int N = L.N, Lt = tiny_lanes(N);
    const int i = threadIdx.x / Lt, sub = threadIdx.x % Lt;
    const bool valid = i < N, owner = valid && sub == 0;
    const double dg = valid ? L.dA[i + i * N] : 1.0;
    double r = valid ? L.r[i] : 0.0;
    double p = precd == 2 ? r / dg : r;
    double d = 0.0;
    double delta_new = wave_sum(owner ? r * p : 0.0);
    const double delta_0 = delta_new, thresh = tol * tol * delta_0;
    long long it = 0;
    while (it < maxit && delta_new > thresh) {
        const double delta_old = delta_new;
        if (owner) pv[i] = p;
        tiny_sync();
        const double q = lds_densedot_split(L.dA, N, N, i, sub, Lt, valid, pv);
        tiny_sync();
        const double alpha = delta_old / wave_sum(owner ? q * p : 0.0);
        d += alpha * p;
        r -= alpha * q;
        const double w = precd == 2 ? r / dg : r;
        delta_new = wave_sum(owner ? r * w : 0.0);
        p = w + (delta_new / delta_old) * p;
        ++it;
    }
    if (owner) L.e[i] = d;
    tiny_sync();
    c.zeromask &= ~(1u << k);
}

// sub-cycle rooted at level k0 >= k_tiny (r_{k0} is in LDS); executed by wave 0 only
__device__ __forceinline__ void tiny_cycle(SolveCtx& c, int k0, bool keep0) {
    const int J = c.D->J, nu = c.D->nu, wc = c.D->wcycle, isnsp = c.D->isnsp, t = threadIdx.x;
    unsigned visited = 0;
    int k = k0;
    bool entering = true, keep = keep0;
    for (int guard = 0; guard < (1 << 22); ++guard) {
        if (entering) {
            if (k == J) {
                SOL_DBG_T0(c);
                tiny_pcg(c, J);
                SOL_DBG_ADD(c, 10);
                if (k == k0) return;
                entering = false;
                k = J - 1;
                continue;
            }
            LdsLevel L = lds_level(c, k);
            if (L.poly) {   // polynomial form: sweeps, residual and restriction in one pass
                SOL_DBG_T0(c);
                poly_pre(c, k, L, keep);
                SOL_DBG_ADD(c, 9);
                visited &= ~(1u << (k + 1));
                k = k + 1;
                keep = false;
                continue;
            }
            if (!keep) {
                c.zeromask |= (1u << k);
                if (nu == 0) {
                    if (t < L.N) L.e[t] = 0.0;
                    tiny_sync();
                    c.zeromask &= ~(1u << k);
                }
            }
            {
                SOL_DBG_T0(c);
                tiny_sweeps(c, k, L, nu, isnsp);
                SOL_DBG_ADD(c, 9);
            }
            {   // residual, then restriction into the child's right-hand side
                SOL_DBG_T0(c);
                {
                    const int Lt = tiny_lanes(L.N), i = t / Lt, sub = t % Lt;
                    const bool valid = i < L.N;
                    const double sd = lds_densedot_split(L.dA, L.N, L.N, i, sub, Lt, valid, L.e);
                    if (valid && sub == 0) L.e2[i] = L.r[i] - sd;   // e2 is free between the sweeps
                }
                tiny_sync();
                {
                    const int Lt = tiny_lanes(L.Nc), i = t / Lt, sub = t % Lt;
                    const bool cv = i < L.Nc;
                    const double rc = lds_densedot_split(L.dPt, L.Nc, L.N, i, sub, Lt, cv, L.e2);
                    if (cv && sub == 0) L.rc[i] = rc;
                }
                tiny_sync();
                SOL_DBG_ADD(c, 11);
            }
            visited &= ~(1u << (k + 1));
            k = k + 1;
            keep = false;
        } else {
            const bool again = wc && (k + 1 < J) && !((visited >> (k + 1)) & 1u);
            if (again) {
                visited |= (1u << (k + 1));
                k = k + 1;
                keep = true;
                entering = true;
                continue;
            }
            LdsLevel L = lds_level(c, k);
            if (L.poly) {   // polynomial form: prolongation and post-smoothing in one pass
                SOL_DBG_T0(c);
                poly_post(c, k, L, lds_e(c, k + 1));
                SOL_DBG_ADD(c, 9);
                if (k == k0) return;
                k = k - 1;
                continue;
            }
            {
                SOL_DBG_T0(c);
                const int Lt = tiny_lanes(L.N), i = t / Lt, sub = t % Lt;
                const bool valid = i < L.N;
                const double sd = lds_densedot_split(L.dP, L.N, L.Nc, i, sub, Lt, valid, lds_e(c, k + 1));
                if (valid && sub == 0) L.e[i] = L.e[i] + sd;
                tiny_sync();
                SOL_DBG_ADD(c, 12);
            }
            {
                SOL_DBG_T0(c);
                tiny_sweeps(c, k, L, nu, isnsp);
                SOL_DBG_ADD(c, 9);
            }
            if (k == k0) return;
            k = k - 1;
        }
    }
}

// ---- block-level sub-cycle: cached levels with <= 1024 rows, one thread per row ---------
// The generic phases (L lanes per row, staging, batched loads) are built for levels that need
// many CUs; on a 100..1000-row level that already sits in LDS they are all fixed cost (~3 us
// a phase, measured).  Here thread i owns row i, a sweep is one row walk and ONE barrier: the
// per-wave partial sums of (A1)'e that the kernel-space correction of the NEXT sweep needs
// are published by the same barrier that publishes the new iterate.
// Lane map of a thread-per-row level.  With a uniform number of lanes per row (lanes_per_row) a
// sweep lasts as long as its longest row -- the coarse levels have hub rows of 60-100 entries against a
// mean of 6 -- and short rows leave most lanes of their group idle.  k_pack_lmap deals the BT lanes
// to the rows by length instead: a row of len entries gets 2^c lanes (c <= 4) so that no lane holds
// more than E entries, with E the smallest of 2, 4, 8, ... for which the rows fit in BT lanes; groups
// are sorted by size (aligned to their size, inside one 16-lane DPP row).  With E <= 4 the lane's
// entries stay in registers for all sweeps of a visit and a sweep's row walk is ONE trip of gathers.
struct LaneSlot {
    int row, sub, lg;
    bool valid;
};
__device__ __forceinline__ LaneSlot lane_slot(AS3 const unsigned* lmap) {
    const unsigned w = lmap[threadIdx.x];
    LaneSlot s;
    s.valid = (w >> 31) != 0;
    s.row = (int)(w & 1023u);
    s.sub = (int)((w >> 10) & 15u);
    s.lg = (int)((w >> 14) & 7u);
    return s;
}
// sum over the lane's group of 2^lg lanes (lg differs from lane to lane), result in every lane of it
__device__ __forceinline__ double subsum_var(double v, int lg) {
    double t = dpp_get<0xB1, 0xf>(v);
    v += lg >= 1 ? t : 0.0;
    t = dpp_get<0x4E, 0xf>(v);
    v += lg >= 2 ? t : 0.0;
    t = dpp_get<0x141, 0xf>(v);
    v += lg >= 3 ? t : 0.0;
    t = dpp_get<0x140, 0xf>(v);
    v += lg >= 4 ? t : 0.0;
    return v;
}
// row walk of a mapped lane in a loop (rows beyond the register budget, and the residual phase)
__device__ __forceinline__ double lds_rowdot_mapped(AS3 const int* ci, AS3 const double* va, int beg, int end,
                                                    const LaneSlot& m, AS3 const double* x) {
    const int Lr = 1 << m.lg;
    double s = 0.0;
    for (int t = beg + m.sub; t < end; t += 4 * Lr) {
        int c[4];
        double v[4], xv[4];
        bool k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int tu = t + u * Lr;
            k[u] = tu < end;
            c[u] = ci[k[u] ? tu : t];
            v[u] = va[k[u] ? tu : t];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k[u]) s += v[u] * xv[u];
    }
    return subsum_var(s, m.lg);
}

// dense thread-per-row level: the lane's part of row i (columns sub + Lr q) from the row-major dense copy
// (leading dimension bdense_ld: whole groups of four q, and rows of a wave on different banks), and its
// dot product with an LDS vector.  No index tests: the copy's and the vectors' padding are zeros
// (bdense_pad entries, see pack_image), so a group of four q is four loads at constant offsets.
// (BDENSE_Q values per lane, ipd_limits.h)
struct DenseRow {
    double v[BDENSE_Q];
};
template <int LR>
__device__ __forceinline__ void dense_row_load_t(AS3 const double* dA, int N, int i, int sub, DenseRow& R) {
    const int Q = bdense_pad(N) / LR;   // a multiple of 4
    AS3 const double* row = dA + i * bdense_ld(N) + sub;
#pragma unroll
    for (int q0 = 0; q0 < BDENSE_Q; q0 += 4) {
        const bool in = q0 < Q;   // uniform
#pragma unroll
        for (int u = 0; u < 4; ++u) R.v[q0 + u] = in ? row[LR * (q0 + u)] : 0.0;
    }
}
template <int LR>
__device__ __forceinline__ double dense_row_dot_t(const DenseRow& R, int N, int sub, AS3 const double* x) {
    const int Q = bdense_pad(N) / LR;
    AS3 const double* xs = x + sub;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int q0 = 0; q0 < BDENSE_Q; q0 += 8) {
        if (q0 >= Q) break;   // uniform
        const double x0 = xs[LR * q0], x1 = xs[LR * (q0 + 1)], x2 = xs[LR * (q0 + 2)], x3 = xs[LR * (q0 + 3)];
        s0 += R.v[q0] * x0;
        s1 += R.v[q0 + 1] * x1;
        s2 += R.v[q0 + 2] * x2;
        s3 += R.v[q0 + 3] * x3;
        if (q0 + 4 >= Q) break;   // uniform
        const double x4 = xs[LR * (q0 + 4)], x5 = xs[LR * (q0 + 5)], x6 = xs[LR * (q0 + 6)], x7 = xs[LR * (q0 + 7)];
        s0 += R.v[q0 + 4] * x4;
        s1 += R.v[q0 + 5] * x5;
        s2 += R.v[q0 + 6] * x6;
        s3 += R.v[q0 + 7] * x7;
    }
    return subwave_sum((s0 + s1) + (s2 + s3), LR);
}
// (row i < N: the caller passes row 0 for lanes without a row and ignores their sum)
__device__ __forceinline__ void dense_row_load(AS3 const double* dA, int N, int i, int sub, DenseRow& R) {
    if (bdense_lanes(N) == 4) dense_row_load_t<4>(dA, N, i, sub, R);
    else dense_row_load_t<8>(dA, N, i, sub, R);
}
__device__ __forceinline__ double dense_row_dot(const DenseRow& R, int N, int sub, AS3 const double* x) {
    return bdense_lanes(N) == 4 ? dense_row_dot_t<4>(R, N, sub, x) : dense_row_dot_t<8>(R, N, sub, x);
}

// ---- block-wide polynomial form ----------------------------------------------------------------
// A visit of a 49..144-row level as ten sweeps, a residual, a restriction and a prolongation is ~13 us
// of barriers and short row walks (a sweep is ~1 us whatever the row count).  In polynomial form
// (SolveLevel::gM) it is two passes y = [Mr | Me | Mc] [r; e; e_c] + W (1'r) like the one-wave levels',
// executed by the whole block: wave w takes the columns 8 b + w, lane l the rows 2 l, 2 l + 1 (and
// 128 + those), i.e. one 16-byte load per column from L2 -- U of them in flight per lane --, the
// eight waves' partial sums meet in LDS.  x is read as a wave-uniform broadcast.
template <int HALVES>
__device__ __forceinline__ void bpoly_pass_t(SolveCtx& c, int k, const double* __restrict__ Mgen,
                                             const double* __restrict__ Wgen, int rows, int nb0,
                                             AS3 const double* x0, int nb1, AS3 const double* x1, int nb2,
                                             AS3 const double* x2, bool pre, AS3 double* outA, int nA,
                                             AS3 double* outB) {
    typedef const __attribute__((address_space(1))) double* gptr;
    typedef __attribute__((ext_vector_type(2))) double d2;
    typedef const __attribute__((address_space(1))) d2* gptr2;
    constexpr int LD = 128 * HALVES, U = HALVES == 1 ? 12 : 8;
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    AS3 double* part = as_lds(c.D->bp_part);
    const bool a0 = 2 * l < rows, a1 = HALVES > 1 && 128 + 2 * l < rows;
    const int nbt = (c.D->dbg_skip & 1) ? 0 : nb0 + nb1 + nb2;
    gptr W = (gptr)Wgen;
    const double wv = t < rows ? W[t] : 0.0;
    // lane j holds x of this wave's j-th column (8 j + w of the concatenated [x0; x1; x2]): the loop
    // below reads it back as a scalar -- no branch on the segment, and 1'x0 is one wave sum
    double xl = 0.0;
    if (l < nbt) {
        AS3 const double* xs = l < nb0 ? x0 + 8 * l : (l < nb0 + nb1 ? x1 + 8 * (l - nb0) : x2 + 8 * (l - nb0 - nb1));
        xl = xs[w];
    }
    const double sx = pre ? wave_sum(l < nb0 ? xl : 0.0) : 0.0;
    const int xlo = __double2loint(xl), xhi = __double2hiint(xl);
    gptr col = (gptr)Mgen + (size_t)w * LD;   // uniform; column 8 b + w starts at col + b * 8 * LD
    double y00 = 0.0, y01 = 0.0, y10 = 0.0, y11 = 0.0;
    if (a0) {
        for (int b0 = 0; b0 < nbt; b0 += U) {
            d2 m0[U], m1[U];
            double xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int b = b0 + u < nbt ? b0 + u : nbt - 1;   // uniform (the surplus of the last batch: x = 0)
                const double x = __hiloint2double(__builtin_amdgcn_readlane(xhi, b), __builtin_amdgcn_readlane(xlo, b));
                xv[u] = b0 + u < nbt ? x : 0.0;
                gptr p = col + (size_t)b * (8 * LD);
                m0[u] = *reinterpret_cast<gptr2>(p + 2 * l);
                if (HALVES > 1) {
                    m1[u] = d2{0.0, 0.0};
                    if (a1) m1[u] = *reinterpret_cast<gptr2>(p + 128 + 2 * l);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                y00 = __builtin_fma(m0[u].x, xv[u], y00);
                y01 = __builtin_fma(m0[u].y, xv[u], y01);
                if (HALVES > 1) {
                    y10 = __builtin_fma(m1[u].x, xv[u], y10);
                    y11 = __builtin_fma(m1[u].y, xv[u], y11);
                }
            }
        }
    }
    part[w * LD + 2 * l] = y00;
    part[w * LD + 2 * l + 1] = y01;
    if (HALVES > 1) {
        part[w * LD + 128 + 2 * l] = y10;
        part[w * LD + 128 + 2 * l + 1] = y11;
    }
    if (pre && l == 0) part[8 * LD + w] = sx;
    __syncthreads();
    double sumr;
    if (pre) {
        sumr = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) sumr += part[8 * LD + g];
        if (t == 0) as_lds(c.sumr)[k] = sumr;   // 1'r of this visit: the post-smoothing pass needs it again
    } else {
        sumr = as_lds(c.sumr)[k];
    }
    if (t < rows) {
        double y = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) y += part[g * LD + t];
        y = __builtin_fma(wv, sumr, y);
        if (t < nA)
            outA[t] = y;
        else
            outB[t - nA] = y;
    }
    __syncthreads();
}
// The same pass with the operators in LDS (SolveLevel::pMr ..., leading dimension 64, one row per lane):
// levels of <= 48 rows whose stacked operator has more than 32 rows.  In ONE wave such a pass has one
// lane per row walk ~100 columns (1.5 us, measured); eight waves take 12 columns each.
__device__ __forceinline__ void lpoly_pass(SolveCtx& c, int k, AS3 const double* M, AS3 const double* W, int rows,
                                           int nb0, AS3 const double* x0, int nb1, AS3 const double* x1, int nb2,
                                           AS3 const double* x2, bool pre, AS3 double* outA, int nA,
                                           AS3 double* outB) {
    constexpr int LD = 64, U = 8;
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    AS3 double* part = as_lds(c.D->bp_part);
    const int nbt = (c.D->dbg_skip & 1) ? 0 : nb0 + nb1 + nb2;
    double xl = 0.0;
    if (l < nbt) {
        AS3 const double* xs = l < nb0 ? x0 + 8 * l : (l < nb0 + nb1 ? x1 + 8 * (l - nb0) : x2 + 8 * (l - nb0 - nb1));
        xl = xs[w];
    }
    const double sx = pre ? wave_sum(l < nb0 ? xl : 0.0) : 0.0;
    const int xlo = __double2loint(xl), xhi = __double2hiint(xl);
    AS3 const double* col = M + w * LD + l;   // column 8 b + w: col + b * 8 * LD (rows beyond `rows` are zeros)
    double y0 = 0.0, y1 = 0.0;
    for (int b0 = 0; b0 < nbt; b0 += U) {
        double m[U], xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int b = b0 + u < nbt ? b0 + u : nbt - 1;   // uniform
            const double x = __hiloint2double(__builtin_amdgcn_readlane(xhi, b), __builtin_amdgcn_readlane(xlo, b));
            xv[u] = b0 + u < nbt ? x : 0.0;
            m[u] = col[b * (8 * LD)];
        }
#pragma unroll
        for (int u = 0; u < U; u += 2) {
            y0 = __builtin_fma(m[u], xv[u], y0);
            y1 = __builtin_fma(m[u + 1], xv[u + 1], y1);
        }
    }
    part[w * LD + l] = y0 + y1;
    if (pre && l == 0) part[8 * LD + w] = sx;
    __syncthreads();
    double sumr;
    if (pre) {
        sumr = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) sumr += part[8 * LD + g];
        if (t == 0) as_lds(c.sumr)[k] = sumr;
    } else {
        sumr = as_lds(c.sumr)[k];
    }
    if (t < rows) {
        double y = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) y += part[g * LD + t];
        y = __builtin_fma(W[t], sumr, y);
        if (t < nA)
            outA[t] = y;
        else
            outB[t - nA] = y;
    }
    __syncthreads();
}
// The block-wide pass of bpoly_pass_t<1> with the operator in LDS (SolveDesc::bm_src: bm_ld rows per column, at
// most 128): the same columns per wave, the same rows per lane, the same order of the sums -- the same bits.
__device__ __forceinline__ void bpoly_pass_lds(SolveCtx& c, int k, AS3 const double* M, int LDm,
                                               AS3 const double* Wl, int rows, int nb0,
                                               AS3 const double* x0, int nb1, AS3 const double* x1, int nb2,
                                               AS3 const double* x2, bool pre, AS3 double* outA, int nA,
                                               AS3 double* outB) {
    typedef __attribute__((ext_vector_type(2))) double d2;
    typedef AS3 const d2* lptr2;
    constexpr int LD = 128, U = 12;
    const int t = threadIdx.x, l = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    AS3 double* part = as_lds(c.D->bp_part);
    const bool a0 = 2 * l < rows;
    const int nbt = (c.D->dbg_skip & 1) ? 0 : nb0 + nb1 + nb2;
    const double wv = t < rows ? Wl[t] : 0.0;
    double xl = 0.0;
    if (l < nbt) {
        AS3 const double* xs = l < nb0 ? x0 + 8 * l : (l < nb0 + nb1 ? x1 + 8 * (l - nb0) : x2 + 8 * (l - nb0 - nb1));
        xl = xs[w];
    }
    const double sx = pre ? wave_sum(l < nb0 ? xl : 0.0) : 0.0;
    const int xlo = __double2loint(xl), xhi = __double2hiint(xl);
    AS3 const double* col = M + w * LDm;   // uniform; column 8 b + w starts at col + b * 8 * LDm
    double y00 = 0.0, y01 = 0.0;
    if (a0) {
        for (int b0 = 0; b0 < nbt; b0 += U) {
            d2 m0[U];
            double xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int b = b0 + u < nbt ? b0 + u : nbt - 1;   // uniform (the surplus of the last batch: x = 0)
                const double x = __hiloint2double(__builtin_amdgcn_readlane(xhi, b), __builtin_amdgcn_readlane(xlo, b));
                xv[u] = b0 + u < nbt ? x : 0.0;
                m0[u] = *reinterpret_cast<lptr2>(col + b * (8 * LDm) + 2 * l);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                y00 = __builtin_fma(m0[u].x, xv[u], y00);
                y01 = __builtin_fma(m0[u].y, xv[u], y01);
            }
        }
    }
    part[w * LD + 2 * l] = y00;
    part[w * LD + 2 * l + 1] = y01;
    if (pre && l == 0) part[8 * LD + w] = sx;
    __syncthreads();
    double sumr;
    if (pre) {
        sumr = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) sumr += part[8 * LD + g];
        if (t == 0) as_lds(c.sumr)[k] = sumr;   // 1'r of this visit: the post-smoothing pass needs it again
    } else {
        sumr = as_lds(c.sumr)[k];
    }
    if (t < rows) {
        double y = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) y += part[g * LD + t];
        y = __builtin_fma(wv, sumr, y);
        if (t < nA)
            outA[t] = y;
        else
            outB[t - nA] = y;
    }
    __syncthreads();
}
__device__ __forceinline__ void bpoly_pass(SolveCtx& c, int k, const LdsLevel& L, int rows, int nb0,
                                           AS3 const double* x0, int nb1, AS3 const double* x1, int nb2,
                                           AS3 const double* x2, bool pre, AS3 double* outA, int nA,
                                           AS3 double* outB) {
    if (L.gM && L.bM)
        bpoly_pass_lds(c, k, L.bM, L.bLD, L.bW, rows, nb0, x0, nb1, x1, nb2, x2, pre, outA, nA, outB);
    else if (!L.gM)
        lpoly_pass(c, k, L.pMr, L.pW, rows, nb0, x0, nb1, x1, nb2, x2, pre, outA, nA, outB);
    else if (L.gLD == 128)
        bpoly_pass_t<1>(c, k, L.gM, L.gW, rows, nb0, x0, nb1, x1, nb2, x2, pre, outA, nA, outB);
    else
        bpoly_pass_t<2>(c, k, L.gM, L.gW, rows, nb0, x0, nb1, x1, nb2, x2, pre, outA, nA, outB);
}
// pre-smoothing, residual and restriction: [e2; r_c] <- Mr r (+ Me e when the visit starts from an iterate)
__device__ __forceinline__ void bpoly_pre(SolveCtx& c, int k, LdsLevel& L, bool keep) {
    const int N = L.N, nb = (N + 7) >> 3;
    bpoly_pass(c, k, L, N + L.Nc, nb, L.r, keep ? nb : 0, L.e, 0, L.e, true, L.e2, N, L.rc);
    AS3 double* tt = L.e;
    L.e = L.e2;
    L.e2 = tt;
    c.swapmask ^= (1u << k);
    c.zeromask &= ~(1u << k);
}
// prolongation + post-smoothing: e2 <- M2a r + M1 e + (M1 P) e_c
__device__ __forceinline__ void bpoly_post(SolveCtx& c, int k, LdsLevel& L, AS3 const double* ec) {
    const int N = L.N, nb = (N + 7) >> 3;
    bpoly_pass(c, k, L, N, nb, L.r, nb, L.e, (L.Nc + 7) >> 3, ec, false, L.e2, N, L.e2);
    AS3 double* tt = L.e;
    L.e = L.e2;
    L.e2 = tt;
    c.swapmask ^= (1u << k);
}

__device__ __forceinline__ double blk_total(AS3 const double* part) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < BT / 64; ++w) s += part[w];
    return s;
}
__device__ __forceinline__ void blk_publish(double v, AS3 double* part) {
    const double w = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
}

// cur: index (0/1) of the partial-sum buffer that describes the current iterate
__device__ __forceinline__ void blk_sweeps(SolveCtx& c, int k, LdsLevel& L, int nu, int isnsp,
                                           int& cur) {
    const int N = L.N;
    // semi-cached level: short rows (<= 12 entries on average: level 2 of a realistic hierarchy) stay
    // thread-per-row with the first entries in registers, long rows are walked from L2 by Lr lanes
    const bool semi_long = L.semi && L.grp[N] > 12 * N;
    const bool semi_regs = L.semi && !semi_long;
    const bool bdense = L.bdense && !L.semi;
    const bool mapped = L.mapped && !L.semi && !bdense;
    LaneSlot ms;
    ms.row = ms.sub = ms.lg = 0;
    ms.valid = false;
    int mapE = 0;
    if (mapped) {
        ms = lane_slot(L.lmap);
        mapE = (int)L.lmap[BT];
    }
    const int Lr = mapped ? (1 << ms.lg) : (semi_regs ? 1 : lanes_per_row(N));
    const int i = mapped ? ms.row : threadIdx.x / Lr, sub = mapped ? ms.sub : threadIdx.x % Lr;
    const bool valid = mapped ? ms.valid : i < N, owner = valid && sub == 0;
    AS3 double* part = as_lds(c.part);
    const double rv = valid ? L.r[i] : 0.0;
    const double ax = valid ? lvl_axi(L, i) : 0.0;
    const double dv = valid ? lvl_dinv(L, i) : 0.0;
    const double sumr = isnsp ? as_lds(c.sumr)[k] : 0.0;
    SemiRow R;
    if (semi_regs) R = semi_row_load(L, i, valid);
    int rbeg = 0, rend = 0;            // entry range of the row: the same for every sweep of the visit
    if (!L.semi && !bdense && valid) {
        rbeg = L.rp[i];
        rend = L.rp[i + 1];
    }
    DenseRow DR;                       // dense levels: the lane's part of the row; lane-map levels: its entries' values
    double* const mv = DR.v;
    if (bdense) dense_row_load(L.dA, N, valid ? i : 0, sub, DR);
    if (semi_long && valid) {
        rbeg = L.grp[i];
        rend = L.grp[i + 1];
    }
    // mapped level with at most sixteen entries per lane: they stay in registers for the visit
    const bool mregs = mapped && mapE >= 1 && mapE <= 16;
    const bool mregs8 = mregs && mapE > 4, mregs16 = mregs && mapE > 8;
    int mc[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) mc[u] = 0;
    if (!bdense) {
#pragma unroll
        for (int u = 0; u < 16; ++u) mv[u] = 0.0;
    }
    if (mregs) {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if ((u >= 4 && !mregs8) || (u >= 8 && !mregs16)) break;
            const int t = rbeg + sub + u * Lr;
            const bool in = valid && t < rend;
            mc[u] = in ? L.ci[t] : 0;
            mv[u] = in ? L.va[t] : 0.0;
        }
    }
    // more than two entries per lane on average: four per trip (one dependent LDS round trip less per
    // sweep on such levels; with two or fewer the masked slots of a wider batch only cost issue slots)
    const bool wide = !L.semi && !bdense && L.rp[N] > 2 * N * Lr;
    const int dskip = c.D->dbg_skip;
    if (dskip & 8) nu = 0;
    for (int s = 0; s < nu; ++s) {
        const bool ez = (c.zeromask >> k) & 1u || (dskip & 4);
        const double eo = (valid && !ez) ? L.e[i] : 0.0;
        double cc = 0.0;
        if (isnsp) cc = (sumr - (ez ? 0.0 : blk_total(part + 16 * cur))) / L.xx;
        double sd = 0.0;
        if (!ez) {
            if (bdense) {
                sd = dense_row_dot(DR, N, sub, L.e);
            } else if (mregs) {
                const double x0 = L.e[mc[0]], x1 = L.e[mc[1]], x2 = L.e[mc[2]], x3 = L.e[mc[3]];
                double acc = (mv[0] * x0 + mv[1] * x1) + (mv[2] * x2 + mv[3] * x3);
                if (mregs8) {
                    const double x4 = L.e[mc[4]], x5 = L.e[mc[5]], x6 = L.e[mc[6]], x7 = L.e[mc[7]];
                    acc += (mv[4] * x4 + mv[5] * x5) + (mv[6] * x6 + mv[7] * x7);
                }
                if (mregs16) {
                    double xx8[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) xx8[u] = L.e[mc[8 + u]];
                    acc += ((mv[8] * xx8[0] + mv[9] * xx8[1]) + (mv[10] * xx8[2] + mv[11] * xx8[3])) +
                           ((mv[12] * xx8[4] + mv[13] * xx8[5]) + (mv[14] * xx8[6] + mv[15] * xx8[7]));
                }
                sd = subsum_var(acc, ms.lg);
            } else if (mapped) {
                sd = lds_rowdot_mapped(L.ci, L.va, rbeg, rend, ms, L.e);
            } else {
                sd = semi_regs   ? semi_row_dot(L, R, L.e)
                     : semi_long ? glb_rowdot_range(L.gci, L.gva, rbeg, rend, sub, Lr, L.e)
                     : wide      ? lds_rowdot_range<4>(L.ci, L.va, rbeg, rend, sub, Lr, L.e)
                                 : lds_rowdot_range<2>(L.ci, L.va, rbeg, rend, sub, Lr, L.e);
            }
        }
        const double v = eo + dv * (rv - sd - ax * cc) + cc;
        if (owner) L.e2[i] = v;
        if (isnsp) blk_publish(owner ? ax * v : 0.0, part + 16 * (cur ^ 1));
        // (per-sweep stamps stood here: c 0.14 | row walk + update 0.53 | publish 0.12 | barrier 0.17 us
        // on a 324/102/34/11 sub-hierarchy; four uniform branches per sweep in a loop that is bound by
        // instruction issue -- ~250 instructions per wave and sweep -- so they were taken out again)
        __syncthreads();
        cur ^= 1;
        AS3 double* t = L.e;
        L.e = L.e2;
        L.e2 = t;
        c.swapmask ^= (1u << k);
        c.zeromask &= ~(1u << k);
    }
}

// sub-cycle rooted at level k0 (k_blk <= k0); r_{k0} is in LDS.  Executed by the whole block.
__device__ __forceinline__ void blk_cycle(SolveCtx& c, int k0, bool keep0) {
    const SolveDesc* D = c.D;
    const int J = D->J, nu = D->nu, isnsp = D->isnsp, wc = D->wcycle, k_tiny = D->k_tiny;
    const int i = threadIdx.x;
    AS3 double* part = as_lds(c.part);
    unsigned visited = 0;
    int k = k0, cur = 0;
    bool entering = true, keep = keep0;
    for (int guard = 0; guard < (1 << 22); ++guard) {
        if (entering && k >= k_tiny) {   // <= 32 rows from here down: wave 0 alone
            SOL_DBG_T0(c);
            if (threadIdx.x < 64) {
                SolveCtx t = c;
                tiny_cycle(t, k, keep);
            }
            __syncthreads();
            SOL_DBG_ADD(c, 4);
            c.zeromask &= ~(1u << k);
            if (k == k0) return;
            entering = false;
            k = k - 1;
            continue;
        }
        if (entering) {
            if (k == J) {   // coarsest level with more than 64 rows
                PcgArgs a = D->pcg;
                a.rhs = D->L[J].lv.r;
                a.d = sol_e(c, J);
                pcg_block(a, c.red);
                __syncthreads();
                c.zeromask &= ~(1u << J);
                if (J == k0) return;
                entering = false;
                k = J - 1;
                continue;
            }
            LdsLevel L = lds_level(c, k);
            if (L.gM || L.poly) {   // block-wide polynomial form: sweeps, residual and restriction in one pass
                SOL_DBG_T0(c);
                bpoly_pre(c, k, L, keep);
                SOL_DBG_ADD(c, 5);
                visited &= ~(1u << (k + 1));
                k = k + 1;
                keep = false;
                continue;
            }
            const bool valid = i < L.N;
            if (!keep) {
                c.zeromask |= (1u << k);
                if (nu == 0) {
                    if (valid) L.e[i] = 0.0;
                    c.zeromask &= ~(1u << k);
                }
            }
            if (isnsp) {   // 1'r of this visit, and (A1)'e when the visit starts from an iterate
                const bool ez = (c.zeromask >> k) & 1u;
                blk_publish(valid ? L.r[i] : 0.0, part + 32);
                blk_publish((valid && !ez) ? lvl_axi(L, i) * L.e[i] : 0.0, part + 16 * cur);
                __syncthreads();
                if (i == 0) as_lds(c.sumr)[k] = blk_total(part + 32);
                __syncthreads();
            } else if (nu == 0) {
                __syncthreads();
            }
            {
                SOL_DBG_T0(c);
                blk_sweeps(c, k, L, nu, isnsp, cur);
                SOL_DBG_ADD(c, 5);
            }
            {   // residual, then restriction into the child's right-hand side
                SOL_DBG_T0(c);
                if (L.bdense && !L.semi) {
                    const int Lr = lanes_per_row(L.N), row = i / Lr, sub = i % Lr;
                    const bool rvld = row < L.N;
                    DenseRow DR;
                    dense_row_load(L.dA, L.N, rvld ? row : 0, sub, DR);
                    const double sd = dense_row_dot(DR, L.N, sub, L.e);
                    if (rvld && sub == 0) L.e2[row] = L.r[row] - sd;
                } else if (L.mapped && !L.semi) {
                    const LaneSlot ms = lane_slot(L.lmap);
                    const int rb = ms.valid ? L.rp[ms.row] : 0, re = ms.valid ? L.rp[ms.row + 1] : 0;
                    const double sd = lds_rowdot_mapped(L.ci, L.va, rb, re, ms, L.e);
                    if (ms.valid && ms.sub == 0) L.e2[ms.row] = L.r[ms.row] - sd;
                } else {
                    const int Lr = lanes_per_row(L.N), row = i / Lr, sub = i % Lr;
                    const bool rvld = row < L.N;
                    const double sd =
                        L.semi ? glb_rowdot_range(L.gci, L.gva, rvld ? L.grp[row] : 0, rvld ? L.grp[row + 1] : 0,
                                                  sub, Lr, L.e)
                               : lds_rowdot_split(L.rp, L.ci, L.va, row, sub, Lr, rvld, L.e);
                    if (rvld && sub == 0) L.e2[row] = L.r[row] - sd;   // e2 is free between the sweeps
                }
                __syncthreads();
                {
                    const int Lr = lanes_per_row(L.Nc), row = i / Lr, sub = i % Lr;
                    const bool cv = row < L.Nc;
                    const double rc =
                        L.semi ? glb_rowdot_split(L.gRrp, L.gRci, L.gRva, row, sub, Lr, cv, L.e2)
                               : lds_rowdot_split(L.Rrp, L.Rci, L.Rva, row, sub, Lr, cv, L.e2);
                    if (cv && sub == 0) L.rc[row] = rc;
                }
                __syncthreads();
                SOL_DBG_ADD(c, 6);
            }
            visited &= ~(1u << (k + 1));
            k = k + 1;
            keep = false;
        } else {
            const bool again = wc && (k + 1 < J) && !((visited >> (k + 1)) & 1u);
            if (again) {
                visited |= (1u << (k + 1));
                k = k + 1;
                keep = true;
                entering = true;
                continue;
            }
            LdsLevel L = lds_level(c, k);
            if (L.gM || L.poly) {   // prolongation and post-smoothing in one pass
                SOL_DBG_T0(c);
                bpoly_post(c, k, L, lds_e(c, k + 1));
                SOL_DBG_ADD(c, 5);
                if (k == k0) return;
                k = k - 1;
                continue;
            }
            SOL_DBG_T0(c);
            {
                const int Lr = lanes_per_row(L.N), row = i / Lr, sub = i % Lr;
                const bool own = row < L.N && sub == 0;
                AS3 const double* ec = lds_e(c, k + 1);
                const double sd =
                    L.semi ? glb_rowdot_split(L.gPrp, L.gPci, L.gPva, row, sub, Lr, row < L.N, ec)
                           : lds_rowdot_split(L.Prp, L.Pci, L.Pva, row, sub, Lr, row < L.N, ec);
                double v = 0.0;
                if (own) {
                    v = L.e[row] + sd;
                    L.e[row] = v;
                }
                if (isnsp) blk_publish(own ? lvl_axi(L, row) * v : 0.0, part + 16 * cur);
                __syncthreads();
            }
            SOL_DBG_ADD(c, 7);
            {
                SOL_DBG_T0(c);
                blk_sweeps(c, k, L, nu, isnsp, cur);
                SOL_DBG_ADD(c, 5);
            }
            if (k == k0) return;
            k = k - 1;
        }
    }
}

// one V or W cycle rooted at level k0 on r_{k0} (in L[k0].lv.r); the correction ends up in
// sol_e(c, k0).  keep0: start from the current iterate of level k0 (MG_Wcycle.m:30).
__device__ __forceinline__ void sol_cycle(SolveCtx& c, int k0 = 1, bool keep0 = false) {
    const SolveDesc* D = c.D;
    const int J = D->J, nu = D->nu;
    unsigned visited = 0;  // bit k: level k has completed one visit under its current parent
    int k = k0;
    bool entering = true, keep = keep0;
    for (int guard = 0; guard < (1 << 22); ++guard) {
        if (entering && k >= D->k_blk) {
            // the whole sub-cycle below here runs thread-per-row out of LDS (wave 0 alone from
            // k_tiny down); 2*nu sweeps per visit leave the e/e2 roles of every level unchanged
            SolveCtx t = c;
            blk_cycle(t, k, keep);
            __syncthreads();
            c.zeromask &= ~(1u << k);
            if (k == k0) return;
            entering = false;
            k = k - 1;
            continue;
        }
        if (entering) {
            if (k == J) {  // coarsest: PCG(A, r)                         MG_Vcycle.m:43
                PcgArgs a = D->pcg;
                a.rhs = D->L[J].lv.r;
                a.d = sol_e(c, J);
                pcg_block(a, c.red);
                __syncthreads();
                c.zeromask &= ~(1u << J);
                if (J == k0) return;
                entering = false;
                k = J - 1;
                continue;
            }
            if (!keep) {
                c.zeromask |= (1u << k);
                if (nu == 0) {  // no sweep will write the iterate: materialise the zero
                    double* e = sol_e(c, k);
                    for (int i = threadIdx.x; i < D->L[k].lv.N; i += BT) e[i] = 0.0;
                    __syncthreads();
                    c.zeromask &= ~(1u << k);
                }
            }
            for (int s = 0; s < nu; ++s) sol_sweep(c, k, false);          // :14-25
            {
                const LevelDev& lv = D->L[k].lv;                          // :27
                phase_resid<true, false>(lv, sol_e(c, k), 0, lv.N, 0, 1, c.lds, c.xs);
                __syncthreads();
                phase_xfer<true>(D->L[k].rest, 0, 1, c.lds, c.xs);
                __syncthreads();
            }
            visited &= ~(1u << (k + 1));
            k = k + 1;
            keep = false;
            entering = true;
        } else {  // back in level k from its child k+1
            const bool again = D->wcycle && (k + 1 < J) && !((visited >> (k + 1)) & 1u);
            if (again) {  // MG_Wcycle.m:30: second correction starting from the first one
                visited |= (1u << (k + 1));
                k = k + 1;
                keep = true;
                entering = true;
                continue;
            }
            XferArgs pa = D->L[k].prol;                                    // :31
            pa.x = sol_e(c, k + 1);
            pa.y = sol_e(c, k);
            phase_xfer<true>(pa, 0, 1, c.lds, c.xs);
            __syncthreads();
            for (int s = 0; s < nu; ++s) sol_sweep(c, k, true);           // :33-41
            if (k == k0) return;
            k = k - 1;
        }
    }
}

__device__ __forceinline__ void sol_top(SolveCtx& c, const double* b, const double* x,
                                        const double* e, double* xnew, double* hist, int first) {
    TopArgs a;
    a.lv = c.D->L[1].lv;
    a.b = b;
    a.x = x;
    a.e = e;
    a.xnew = xnew;
    a.row0 = 0;
    a.row1 = a.lv.N;
    a.staged = 1;
    phase_top<true, false>(a, 0, 1, c.lds, c.xs);
    __syncthreads();
    ConvArgs ca;
    ca.r = a.lv.r;
    ca.n = a.lv.N;
    ca.hist = hist;
    ca.first = first;
    conv_block(ca, c.red);
    __syncthreads();
}

struct PackEntry {
    const void* src;
    unsigned dst_off, bytes;  // multiples of 4
};
// compact copy of a block-wide polynomial operator (column-major, gld rows per column) with ld rows per column
// (SolveDesc::bm_src): one workgroup per column
// (the last workgroup copies the vector W behind the columns)
__global__ __launch_bounds__(128) void k_bm_compact(const double* __restrict__ src, int gld, double* __restrict__ dst,
                                                    int ld, const double* __restrict__ W, int rows) {
    const int c = blockIdx.x, r = threadIdx.x;
    if (c == (int)gridDim.x - 1) {
        if (r < ld) dst[(size_t)c * ld + r] = r < rows ? W[r] : 0.0;
        return;
    }
    if (r < ld) dst[(size_t)c * ld + r] = src[(size_t)c * gld + r];
}
// gathers the constant arrays of the cached levels into the image (one workgroup per array)
__global__ __launch_bounds__(256) void k_pack_image(const PackEntry* __restrict__ ents,
                                                    char* __restrict__ img) {
    const PackEntry e = ents[blockIdx.x];
    const int* src = reinterpret_cast<const int*>(e.src);
    int* dst = reinterpret_cast<int*>(img + e.dst_off);
    for (unsigned i = threadIdx.x; i < e.bytes / 4; i += 256) dst[i] = src[i];
}

struct DenseEntry {
    const int* rp;
    const int* ci;
    const double* va;
    int rows, cols;
    unsigned dst_off;
    int ld_row;   // 0: column-major; > 0: row-major with this leading dimension (dense thread-per-row levels)
};
// dense column-major copies of the tiny levels' operators (one workgroup per matrix)
__global__ __launch_bounds__(256) void k_pack_dense(const DenseEntry* __restrict__ ents,
                                                    char* __restrict__ img) {
    const DenseEntry e = ents[blockIdx.x];
    double* dst = reinterpret_cast<double*>(img + e.dst_off);
    const int total = e.ld_row ? e.rows * e.ld_row : e.rows * e.cols;
    for (int t = threadIdx.x; t < total; t += 256) dst[t] = 0.0;
    __syncthreads();
    for (int r = threadIdx.x; r < e.rows; r += 256)
        for (int t = e.rp[r]; t < e.rp[r + 1]; ++t) {
            if (e.ld_row) dst[(size_t)r * e.ld_row + e.ci[t]] = e.va[t];
            else dst[r + (size_t)e.ci[t] * e.rows] = e.va[t];
        }
}

// Lane map of a thread-per-row level (see blk_sweeps): one workgroup per level.
struct LmapEntry {
    const int* rp;
    int N;
    unsigned off;
};
__global__ __launch_bounds__(BT) void k_pack_lmap(const LmapEntry* __restrict__ ents, char* __restrict__ img) {
    __shared__ int wsum[BT / 64];
    __shared__ int cnt[5], base[5];
    const LmapEntry e = ents[blockIdx.x];
    unsigned* map = reinterpret_cast<unsigned*>(img + e.off);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int len = t < e.N ? e.rp[t + 1] - e.rp[t] : 0;
    auto block_sum = [&](int v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        __syncthreads();
        if (lane == 0) wsum[wv] = v;
        __syncthreads();
        int s = 0;
        for (int w = 0; w < BT / 64; ++w) s += wsum[w];
        return s;
    };
    auto block_max = [&](int v) {
        for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
        __syncthreads();
        if (lane == 0) wsum[wv] = v;
        __syncthreads();
        int s = 0;
        for (int w = 0; w < BT / 64; ++w) s = max(s, wsum[w]);
        return s;
    };
    const int maxlen = block_max(len);
    int E = 2, need = 0;
    for (;; E <<= 1) {
        int n = 1;
        while (n < 16 && n * E < len) n <<= 1;
        need = t < e.N ? n : 0;
        if (block_sum(need) <= BT || E >= (1 << 20)) break;   // (uniform)
    }
    int lg = 0;
    while ((1 << lg) < need) ++lg;
    if (t < 5) cnt[t] = 0;
    map[t] = 0u;
    __syncthreads();
    // rank of the row among the rows of its class, in row order
    int rank = 0;
    for (int c = 0; c < 5; ++c) {
        const bool mine = t < e.N && lg == c;
        const unsigned long long b = __ballot(mine);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < BT / 64; ++w) {
            if (w < wv) woff += wsum[w];
            tot += wsum[w];
        }
        if (mine) rank = woff + before;
        if (t == 0) cnt[c] = tot;
    }
    __syncthreads();
    if (t == 0) {   // classes by descending group size: every group is aligned to its size
        int off = 0;
        for (int c = 4; c >= 0; --c) {
            base[c] = off;
            off += cnt[c] << c;
        }
        map[BT] = (E <= 16 && maxlen <= 16 * E) ? (unsigned)E : 0u;
    }
    __syncthreads();
    if (t < e.N) {
        const int b0 = base[lg] + (rank << lg);
        for (int s = 0; s < (1 << lg); ++s)
            map[b0 + s] = (unsigned)t | ((unsigned)s << 10) | ((unsigned)lg << 14) | (1u << 31);
    }
}

// Polynomial form of a one-wave level (see poly_pre / poly_post): one workgroup per level forms
//   Rg = R + u 1', u = (1 - R A1) / xx (isnsp) or 0 ;  S = I - Rg A ;  M1 = S^nu ;
//   M2 = sum_{j<nu} S^j Rg = M2a + w 1'  with  M2a = sum S^j R ,  w = sum S^j u
//   T1 = P'A ;  Mr = [M2a; P' - T1 M2a] ;  W = [w; -T1 w] ;  Me = [M1; -T1 M1] ;  Mc = M1 P
// with dense column-major matrices in LDS and writes Mr, Me, Mc, W into the image.  The rank-one part
// w 1' stays apart because u ~ 1/xx is large (xx = 1'A1 ~ N bk1): added into every entry of M2 it
// would cost the cancellation inside 1'r that the sweeps' own xig = 1'g enjoys (MG_Vcycle.m:17).
struct PolyEntry {
    const int *Arp, *Aci;
    const double* Ava;
    const int *Prp, *Pci;   // P  : N x Nc  (CSR)
    const double* Pva;
    const double* dinv;
    const double* Axi;
    const double* xx;
    int N, Nc, nu, isnsp, LD;
    unsigned offMr, offMe, offMc, offW;
};
__global__ __launch_bounds__(BT) void k_pack_poly(const PolyEntry* __restrict__ ents, char* __restrict__ img) {
    extern __shared__ __attribute__((aligned(16))) char poly_raw[];
    const PolyEntry e = ents[blockIdx.x];
    const int N = e.N, Nc = e.Nc, R = N + Nc, LD = e.LD, t = threadIdx.x;
    const int N8 = (N + 7) / 8 * 8, Nc8 = (Nc + 7) / 8 * 8;
    double* A = reinterpret_cast<double*>(poly_raw);   // N x N, column-major like everything here
    double* S = A + N * N;
    double* M1 = S + N * N;
    double* M2 = M1 + N * N;                            // M2a
    double* T = M2 + N * N;                             // product scratch
    double* P = T + N * N;                              // N x Nc
    double* T1 = P + N * Nc;                            // Nc x N
    double* u = T1 + Nc * N;                            // N
    double* dv = u + N;                                 // N
    double* w = dv + N;                                 // N
    double* w2 = w + N;                                 // N
    for (int i = t; i < N * N; i += BT) A[i] = 0.0;
    for (int i = t; i < N * Nc; i += BT) P[i] = 0.0;
    __syncthreads();
    for (int r = t; r < N; r += BT) {
        for (int q = e.Arp[r]; q < e.Arp[r + 1]; ++q) A[r + e.Aci[q] * N] = e.Ava[q];
        for (int q = e.Prp[r]; q < e.Prp[r + 1]; ++q) P[r + e.Pci[q] * N] = e.Pva[q];
        const double d = e.dinv[r];
        dv[r] = d;
        u[r] = e.isnsp ? (1.0 - d * e.Axi[r]) / e.xx[0] : 0.0;
        w[r] = 0.0;
    }
    __syncthreads();
    // S = I - Rg A,  (Rg A)[i][j] = dinv_i A[i][j] + u_i (1'A)_j ;  M1 = I ;  M2a = 0 ;  w = 0
    for (int q = t; q < N * N; q += BT) {
        const int i = q % N, j = q / N;
        double cs = 0.0;
        for (int k = 0; k < N; ++k) cs += A[k + j * N];
        S[q] = (i == j ? 1.0 : 0.0) - (dv[i] * A[q] + u[i] * cs);
        M1[q] = i == j ? 1.0 : 0.0;
        M2[q] = 0.0;
    }
    __syncthreads();
    for (int s = 0; s < e.nu; ++s) {
        // M2a <- R + S M2a ;  w <- u + S w ;  M1 <- S M1     (results parked: all read the old values)
        for (int q = t; q < 2 * N * N + N; q += BT) {
            if (q >= 2 * N * N) {
                const int i = q - 2 * N * N;
                double acc = 0.0;
                for (int k = 0; k < N; ++k) acc += S[i + k * N] * w[k];
                w2[i] = u[i] + acc;
                continue;
            }
            const bool second = q >= N * N;
            const int qq = second ? q - N * N : q;
            const int i = qq % N, j = qq / N;
            const double* B = second ? M1 : M2;
            double acc = 0.0;
            for (int k = 0; k < N; ++k) acc += S[i + k * N] * B[k + j * N];
            if (second)
                T[qq] = acc;
            else
                A[qq] = acc + (i == j ? dv[i] : 0.0);   // A is rebuilt below; until then: second scratch
        }
        __syncthreads();
        for (int q = t; q < N * N; q += BT) {
            M1[q] = T[q];
            M2[q] = A[q];
        }
        for (int i = t; i < N; i += BT) w[i] = w2[i];
        __syncthreads();
    }
    // A again (it was scratch), then T1 = P'A
    for (int i = t; i < N * N; i += BT) A[i] = 0.0;
    __syncthreads();
    for (int r = t; r < N; r += BT)
        for (int q = e.Arp[r]; q < e.Arp[r + 1]; ++q) A[r + e.Aci[q] * N] = e.Ava[q];
    __syncthreads();
    for (int q = t; q < Nc * N; q += BT) {
        const int c = q % Nc, j = q / Nc;
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc += P[k + c * N] * A[k + j * N];
        T1[q] = acc;
    }
    __syncthreads();
    double* Mr = reinterpret_cast<double*>(img + e.offMr);
    double* Me = reinterpret_cast<double*>(img + e.offMe);
    double* Mc = reinterpret_cast<double*>(img + e.offMc);
    double* W = reinterpret_cast<double*>(img + e.offW);
    for (int q = t; q < LD * N8; q += BT) {
        const int row = q % LD, j = q / LD;
        double vr = 0.0, ve = 0.0;
        if (j < N && row < N) {
            vr = M2[row + j * N];
            ve = M1[row + j * N];
        } else if (j < N && row < R) {
            const int c = row - N;
            double a2 = 0.0, a1 = 0.0;
            for (int k = 0; k < N; ++k) {
                a2 += T1[c + k * Nc] * M2[k + j * N];
                a1 += T1[c + k * Nc] * M1[k + j * N];
            }
            vr = P[j + c * N] - a2;
            ve = -a1;
        }
        Mr[q] = vr;
        Me[q] = ve;
    }
    for (int q = t; q < LD * Nc8; q += BT) {
        const int i = q % LD, c = q / LD;
        double acc = 0.0;
        if (i < N && c < Nc)
            for (int k = 0; k < N; ++k) acc += M1[i + k * N] * P[k + c * N];
        Mc[q] = acc;
    }
    for (int row = t; row < LD; row += BT) {
        double v = 0.0;
        if (row < N) {
            v = w[row];
        } else if (row < R) {
            const int c = row - N;
            for (int k = 0; k < N; ++k) v += T1[c + k * Nc] * w[k];
            v = -v;
        }
        W[row] = v;
    }
}

// Block-wide polynomial form of a 33..144-row level (SolveLevel::gM): the recurrences of k_pack_poly
// as dense products on the f64 matrix cores.  All operands live in global scratch, column-major, padded
// with zeros to multiples of 16 (Np rows; no edge cases in the tiles).  M1 = S^nu by nu - 1 products
// S^j = S S^(j-1); their running sum I + S + ... + S^(nu-1) gives M2a (columns scaled by D^-1) and w
// (applied to u).  Y = [sum | S^nu | w, 15 zero columns] is one matrix of 2 Np + 16 columns, so that the
// rows below N of the output are one more product, T1 Y.  One wave per 16 x 16 tile
// (v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result
// register g of lane l is C[(l >> 4) + 4 g][l & 15]), the operand loads of 64 k in flight.
struct BPolyEntry {
    const int* Arp;
    const int* Aci;
    const double* Ava;
    const int* Prp;
    const int* Pci;
    const double* Pva;
    const double* dinv;
    const double* Axi;
    const double* xx;
    int N, Nc, Np, Ncp, nu, isnsp, LD;
    double* A;    // Np x Np
    double* S;    // Np x Np
    double* P;    // Np x Ncp
    double* T1;   // Ncp x Np = P'A
    double* Pw[2]; // Np x Np: the powers of S, ping-pong
    double* Y;     // Np x (2 Np + 16): [I + S + ... + S^(nu-1) | S^nu | w, 15 zero columns]
    double* dv;
    double* u;
    double* cs;   // column sums of A
    double* M;    // out: [Mr | Me | Mc], LD rows, 8-padded column counts (zeroed by the host)
    double* W;    // out: LD
    // out, instead of M: row-major [N + Nc][RES_P3_LD] with Mr in columns 0..N-1, Me in 512..512+N-1
    // and Mc in 1024..1024+Nc-1 (the resident kernels' third level: a thread holds entries t, 512 + t
    // and 1024 + t of its workgroup's rows, ipd_resident.h POLY3); W then has N + Nc entries
    double* rows;
    int rows_seg;   // segment length of that layout: 512 (k_resident, Mc at most 128 columns) or RB_P3_SEG
    int rows_ld;    // its row stride
};
typedef double bp_d4 __attribute__((ext_vector_type(4)));
// (the k index of MFMA u in a group of four is k0 + 4 (l >> 4) + u, not k0 + 4 u + (l >> 4): a lane's four
// B values are then 32 contiguous bytes and the four lanes of a column share one 128-byte line -- with
// the natural order every load touched sixteen lines for 32 bytes each and a product of 288^3 took 14 us)
// One tile per WORKGROUP: wave w takes the 16-k groups w, w + 4, ... (a product is a chain of dependent
// batches of loads otherwise: 288 / 64 = 5 round trips to L2), the four partial tiles are added in wave
// order through LDS; the sum is returned to wave 0 only.
__device__ __forceinline__ bp_d4 bp_tile(const double* __restrict__ A, int a_is, int a_ks,
                                         const double* __restrict__ B, int b_ks, int b_js, int K, int I0, int J0) {
    typedef double bp_v2 __attribute__((ext_vector_type(2)));
    __shared__ double bp_part[3][4][64];
    const int l = threadIdx.x & 63, r = l & 15, q = l >> 4, wv = threadIdx.x >> 6;
    const double* ap = A + (size_t)(I0 + r) * a_is + (size_t)(4 * q) * a_ks;
    const double* bp = B + (size_t)(4 * q) * b_ks + (size_t)(J0 + r) * b_js;   // b_ks == 1
    bp_d4 c = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 256) {
        double a[16], b[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = k0 + 16 * (4 * g + wv);
            const bool in = k < K;   // uniform (K is a multiple of 16)
            if (in) {
                const bp_v2 b01 = *reinterpret_cast<const bp_v2*>(bp + k);
                const bp_v2 b23 = *reinterpret_cast<const bp_v2*>(bp + k + 2);
                b[4 * g] = b01.x;
                b[4 * g + 1] = b01.y;
                b[4 * g + 2] = b23.x;
                b[4 * g + 3] = b23.y;
                if (a_ks == 1) {
                    const bp_v2 a01 = *reinterpret_cast<const bp_v2*>(ap + k);
                    const bp_v2 a23 = *reinterpret_cast<const bp_v2*>(ap + k + 2);
                    a[4 * g] = a01.x;
                    a[4 * g + 1] = a01.y;
                    a[4 * g + 2] = a23.x;
                    a[4 * g + 3] = a23.y;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[4 * g + u] = ap[(size_t)(k + u) * a_ks];
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) a[4 * g + u] = b[4 * g + u] = 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (k0 + 16 * (4 * (u / 4) + wv) < K) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], c, 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bp_part[wv - 1][g][l] = c[g];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int ww = 0; ww < 3; ++ww)
#pragma unroll
            for (int g = 0; g < 4; ++g) c[g] += bp_part[ww][g][l];
    }
    return c;
}
// dense copies of A and P, D^-1, u, and the parts of the state after the first sweep that are not S:
// M2a = D^-1, w = u
__global__ __launch_bounds__(256) void k_bpoly_scatter(const BPolyEntry e) {   // one wave per row
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, Np = e.Np;
    if (r >= e.N) return;
    for (int q = e.Arp[r] + lane; q < e.Arp[r + 1]; q += 64) e.A[r + (size_t)e.Aci[q] * Np] = e.Ava[q];
    for (int q = e.Prp[r] + lane; q < e.Prp[r + 1]; q += 64) e.P[r + (size_t)e.Pci[q] * Np] = e.Pva[q];
    if (lane == 0) {
        const double d = e.dinv[r];
        const double ui = e.isnsp ? (1.0 - d * e.Axi[r]) / e.xx[0] : 0.0;
        e.dv[r] = d;
        e.u[r] = ui;
        if (e.nu == 1) e.Y[r + (size_t)(2 * Np) * Np] = ui;   // w = u
    }
}
__global__ __launch_bounds__(256) void k_bpoly_colsum(const BPolyEntry e) {   // one wave per column
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= e.N) return;
    const double* aj = e.A + (size_t)j * e.Np;
    double cs = 0.0;
    for (int k = lane; k < e.N; k += 64) cs += aj[k];
    cs = wave_sum(cs);
    if (lane == 0) e.cs[j] = cs;
}
// S = I - Rg A with (Rg A)[i][j] = dinv_i A[i][j] + u_i (1'A)_j, the first power and the sum so far
// (blocks below nS: one thread per entry); T1 = P'A (the tiles behind)
__global__ __launch_bounds__(256) void k_bpoly_S_T1(const BPolyEntry e, int nS) {
    const int N = e.N, Np = e.Np;
    if ((int)blockIdx.x < nS) {
        const int q = blockIdx.x * 256 + threadIdx.x;
        if (q >= N * N) return;
        const int i = q % N, j = q / N;
        const size_t at = i + (size_t)j * Np;
        const double id = i == j ? 1.0 : 0.0;
        const double sv = id - (e.dv[i] * e.A[at] + e.u[i] * e.cs[j]);
        e.S[at] = sv;
        e.Pw[0][at] = sv;
        e.Y[at] = e.nu >= 2 ? id + sv : id;
        if (e.nu == 1) e.Y[at + (size_t)Np * Np] = sv;
        return;
    }
    const int tile = (int)blockIdx.x - nS, ni = e.Ncp / 16;
    const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni), l = threadIdx.x & 63;
    const bp_d4 c = bp_tile(e.P, Np, 1, e.A, 1, Np, Np, I0, J0);   // A-operand (c, k) = P[k + c Np]
    if (threadIdx.x >= 64) return;
    for (int g = 0; g < 4; ++g) e.T1[(I0 + (l >> 4) + 4 * g) + (size_t)(J0 + (l & 15)) * e.Ncp] = c[g];
}
// S^s = S S^(s-1) (s = 2 .. nu; the last one lands in Y's second block), added to the sum while s < nu;
// beside the last product: w = (I + ... + S^(nu-1)) u, one wave per row
__global__ __launch_bounds__(256) void k_bpoly_step(const BPolyEntry e, int s, int src, int nT) {
    const int Np = e.Np, ni = Np / 16, l = threadIdx.x & 63;
    if ((int)blockIdx.x >= nT) {
        const int i = ((int)blockIdx.x - nT) * 4 + (threadIdx.x >> 6);
        if (i >= e.N) return;
        double acc = 0.0;
        for (int j = l; j < e.N; j += 64) acc += e.Y[i + (size_t)j * Np] * e.u[j];
        acc = wave_sum(acc);
        if (l == 0) e.Y[i + (size_t)(2 * Np) * Np] = acc;
        return;
    }
    const int tile = blockIdx.x;
    const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
    const bp_d4 c = bp_tile(e.S, 1, Np, e.Pw[src], 1, Np, Np, I0, J0);
    if (threadIdx.x >= 64) return;
    double* dst = s == e.nu ? e.Y + (size_t)Np * Np : e.Pw[src ^ 1];
    const int j = J0 + (l & 15);
    for (int g = 0; g < 4; ++g) {
        const size_t at = (size_t)(I0 + (l >> 4) + 4 * g) + (size_t)j * Np;
        dst[at] = c[g];
        if (s < e.nu) e.Y[at] += c[g];
    }
}
// the stacked output: rows below N from -T1 Y (+ P' in the Mr block), Mc = M1 P, copies above
__global__ __launch_bounds__(256) void k_bpoly_final(const BPolyEntry e, int nZ, int nC) {
    const int N = e.N, Nc = e.Nc, Np = e.Np, Ncp = e.Ncp, LD = e.LD, l = threadIdx.x & 63;
    const int N8 = (N + 7) / 8 * 8;
    const double* Y = e.Y;
    auto put = [&](int row, bool me, int j, double v) {
        if (e.rows)
            e.rows[(size_t)row * e.rows_ld + (me ? e.rows_seg : 0) + j] = v;
        else
            e.M[row + (size_t)((me ? N8 : 0) + j) * LD] = v;
    };
    int blk = blockIdx.x;
    if (blk < nZ) {   // Z = T1 Y: Ncp x (2 Np + 16)
        const int ni = Ncp / 16, tile = blk;
        const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
        const bp_d4 c = bp_tile(e.T1, 1, Ncp, Y, 1, Np, Np, I0, J0);
        if (threadIdx.x >= 64) return;
        const int j = J0 + (l & 15);
        for (int g = 0; g < 4; ++g) {
            const int cc = I0 + (l >> 4) + 4 * g;
            if (cc >= Nc) continue;
            if (j < Np) {
                if (j < N) put(N + cc, false, j, e.P[j + (size_t)cc * Np] - c[g] * e.dv[j]);
            } else if (j < 2 * Np) {
                if (j - Np < N) put(N + cc, true, j - Np, -c[g]);
            } else if (j == 2 * Np) {
                e.W[N + cc] = -c[g];
            }
        }
        return;
    }
    blk -= nZ;
    if (blk < nC) {   // Mc = M1 P: Np x Ncp
        const int ni = Np / 16, tile = blk;
        const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
        const bp_d4 c = bp_tile(Y + (size_t)Np * Np, 1, Np, e.P, 1, Np, Np, I0, J0);
        if (threadIdx.x >= 64) return;
        const int j = J0 + (l & 15);
        for (int g = 0; g < 4; ++g) {
            const int i = I0 + (l >> 4) + 4 * g;
            if (i < N && j < Nc) {
                if (e.rows)
                    e.rows[(size_t)i * e.rows_ld + 2 * e.rows_seg + j] = c[g];
                else
                    e.M[i + (size_t)(2 * N8 + j) * LD] = c[g];
            }
        }
        return;
    }
    blk -= nC;
    const int q = blk * 256 + threadIdx.x;   // copies: M2a = sum D^-1, M1, w
    if (q < N * N) {
        const int i = q % N, j = q / N;
        put(i, false, j, Y[i + (size_t)j * Np] * e.dv[j]);
        put(i, true, j, Y[i + (size_t)(Np + j) * Np]);
    } else if (q < N * N + N) {
        const int i = q - N * N;
        e.W[i] = Y[i + (size_t)(2 * Np) * Np];
    }
}

// Level 2 of the resident kernel, composed over a whole visit (ResDesc::p2rows; pack_bpoly in its row layout
// has run): B = M1 M2a + M2a into the Me segment of the rows (tiles below nT), wB = M1 w + w into W (one wave
// per row behind).  M1 = Y's second block, M2a = Y's first block with columns scaled by D^-1, w = Y's column 2 Np.
__global__ __launch_bounds__(256) void k_bpoly_compose(const BPolyEntry e, int nT) {
    const int N = e.N, Np = e.Np, l = threadIdx.x & 63;
    const double* Y = e.Y;
    if ((int)blockIdx.x >= nT) {
        const int i = ((int)blockIdx.x - nT) * 4 + (threadIdx.x >> 6);
        if (i >= N) return;
        double acc = 0.0;
        for (int j = l; j < N; j += 64) acc += Y[i + (size_t)(Np + j) * Np] * Y[j + (size_t)(2 * Np) * Np];
        acc = wave_sum(acc);
        if (l == 0) e.W[i] = acc + Y[i + (size_t)(2 * Np) * Np];
        return;
    }
    const int ni = Np / 16, tile = blockIdx.x;
    const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
    const bp_d4 c = bp_tile(Y + (size_t)Np * Np, 1, Np, Y, 1, Np, Np, I0, J0);
    if (threadIdx.x >= 64) return;
    const int j = J0 + (l & 15);
    for (int g = 0; g < 4; ++g) {
        const int i = I0 + (l >> 4) + 4 * g;
        if (i < N && j < N)
            e.rows[(size_t)i * e.rows_ld + e.rows_seg + j] = (c[g] + Y[i + (size_t)j * Np]) * e.dv[j];
    }
}

__host__ __device__ constexpr size_t sol_r16(size_t b) { return (b + 15) / 16 * 16; }
static_assert(sol_r16(sizeof(SolveDesc)) + sol_r16(4 * RELOC_MAX) == SOL_HEAD, "ipd_limits.h: SOL_HEAD is the image head");

// One flat copy of the image (many 16-byte loads in flight per lane) instead of one dependent
// global round trip per array (measured: ~60 arrays x ~1.5 us dominated the sub-cycle kernel).
__device__ __forceinline__ SolveDesc* sol_load_image(const SolveDesc* Dg, char* dyn_raw) {
    const int stage = Dg->stage_bytes, n16 = Dg->image_bytes / 16;
    const uint4* src = reinterpret_cast<const uint4*>(Dg);
    uint4* dst = reinterpret_cast<uint4*>(dyn_raw + stage);
    for (int i = threadIdx.x; i < n16; i += BT) dst[i] = src[i];
    // the work vectors behind the image start from zero: the polynomial passes read the vectors of the
    // one-wave levels in whole 8-entry blocks, and their padding must stay zero
    {
        const int w16 = (Dg->lds_total - stage - Dg->image_bytes) / 16;
        uint4* wz = dst + n16;
        for (int i = threadIdx.x; i < w16; i += BT) wz[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    SolveDesc* LD = reinterpret_cast<SolveDesc*>(dyn_raw + stage);
    const unsigned* rel =
        reinterpret_cast<const unsigned*>(dyn_raw + stage + sol_r16(sizeof(SolveDesc)));
    for (int t = threadIdx.x; t < LD->nreloc; t += BT) {
        char** f = reinterpret_cast<char**>(reinterpret_cast<char*>(LD) + rel[t]);
        *f = dyn_raw + reinterpret_cast<size_t>(*f);
    }
    __syncthreads();
    return LD;
}

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
    SolveCtx c;
    // without cached levels the descriptor stays in global memory: its (uniform) fields
    // are then fetched with scalar loads and live in SGPRs instead of VGPRs
    c.D = CACHED ? LD : D_global;
    c.lds = &lds;
    c.red = red;
    c.xs = reinterpret_cast<double*>(dyn_raw);
    c.swapmask = 0;
    c.zeromask = 0;
    c.part = blkpart;
    c.sumr = blkpart + 48;
    c.dbg = nullptr;
    c.bm_lds = 0;
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
// the same SolveDesc / LDS image, with M(r) = sol_cycle(c) from a zero guess: one launch and one
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
    SolveCtx c;
    c.D = CACHED ? LD : D_global;
    c.lds = &lds;
    c.red = red;
    c.xs = reinterpret_cast<double*>(dyn_raw);
    c.swapmask = 0;
    c.zeromask = 0;
    c.part = blkpart;
    c.sumr = blkpart + 48;
    c.dbg = nullptr;
    c.bm_lds = 0;
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
    double res = sqrt(fabs(delta / delta0));
    int it = 0;
    while (it < a.maxit && delta > a.tol2 * delta0) {                         // :76
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
        beta = (dn - s_wo) / delta;                                           // flexible :82
        delta = dn;
        ++it;                                                                 // :84
        res = sqrt(fabs(dn / delta0));                                        // :85
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
    SolveCtx c;
    c.D = LD;
    c.lds = &lds;
    c.red = red;
    c.xs = reinterpret_cast<double*>(dyn_raw);
    c.swapmask = 0;
    c.zeromask = 0;
    c.part = blkpart;
    c.sumr = blkpart + 48;
    c.dbg = dbg;
    c.bm_lds = 0;
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

#include "ipd_resident_proto.h"
#include "ipd_resident.h"
#include "ipd_resident_big.h"
#include "ipd_cycle_host.h"
