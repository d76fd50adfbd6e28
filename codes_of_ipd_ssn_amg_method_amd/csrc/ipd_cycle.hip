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

#include "ipd_interp.h"   // and ipd_cycle_args.h, ipd_cycle_pcg.h, ipd_cycle_phases.h, ipd_cycle_dev.h

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

#include "ipd_resident_big.h"   // (and ipd_resident.h: the descriptors; ipd_resident_k*.hip instantiate the kernels)
#include "ipd_cycle_host.h"
