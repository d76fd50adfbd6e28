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
#include "ipd_cycle_state.h"

#include <cmath>

#include "ipd_cycle_pcg.h"

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

__global__ void k_maskop_scales(int nf, int nc, const double* __restrict__ p,
                                const double* __restrict__ q, double itk,
                                double* __restrict__ alpha, double* __restrict__ beta) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nf + nc; t += gridDim.x * blockDim.x) {
        if (t < nf)
            alpha[t] = q[t] * q[t] * itk;
        else
            beta[t - nf] = p[t - nf] * p[t - nf];
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

// All levels of a hierarchy in two launches instead of two per level (the hierarchy is rebuilt at every
// Newton step): workgroup b of k_levels_prepare belongs to the level whose block range holds b, workgroup
// k of k_levels_sum adds A*1 of level k in k_vec_sum's order (same bits).
constexpr int PREP_ML = 24;
struct PrepLevels {
    int n;
    int first_block[PREP_ML + 1];
    int N[PREP_ML], nf[PREP_ML];
    const int* rp[PREP_ML];
    const int* ci[PREP_ML];
    const double* va[PREP_ML];
    double* dinv[PREP_ML];
    double* Axi[PREP_ML];
    double* xx[PREP_ML];
    int* maxoff[PREP_ML];
};
__global__ void k_levels_prepare(const PrepLevels P) {
    int k = 0;
    while (k + 1 < P.n && (int)blockIdx.x >= P.first_block[k + 1]) ++k;
    const int nb = P.first_block[k + 1] - P.first_block[k], lb = blockIdx.x - P.first_block[k];
    const int N = P.N[k], nf = P.nf[k];
    const int* __restrict__ rp = P.rp[k];
    const int* __restrict__ ci = P.ci[k];
    const double* __restrict__ va = P.va[k];
    const int lane = threadIdx.x & 63;
    const int wave = (lb * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (nb * blockDim.x) >> 6;
    int longest = 0;
    for (int r = wave; r < N; r += nwaves) {
        double s = 0.0, dg = 0.0;
        int hasd = 0;
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            s += va[t];
            if (ci[t] == r) {
                dg = va[t];
                hasd = 1;
            }
        }
        s = wave_sum(s);
        dg = wave_sum(dg);
        hasd = __any(hasd) ? 1 : 0;
        longest = max(longest, rp[r + 1] - rp[r] - hasd);
        if (lane == 0) {
            P.Axi[k][r] = s;
            P.dinv[k][r] = nf > 0 ? 1.0 / dg : 0.5 * (1.0 / dg);
        }
    }
    // one atomic per workgroup (one per wave on one address cost 35 of the kernel's 41 us)
    __shared__ int bmax;
    if (threadIdx.x == 0) bmax = 0;
    __syncthreads();
    if (lane == 0 && longest > 0) atomicMax(&bmax, longest);
    __syncthreads();
    if (threadIdx.x == 0 && bmax > 0) atomicMax(P.maxoff[k], bmax);
}
__global__ __launch_bounds__(BT) void k_levels_sum(const PrepLevels P) {
    __shared__ double red[16];
    const int k = blockIdx.x;
    const double* v = P.Axi[k];
    double s = 0.0;
    for (int t = threadIdx.x; t < P.N[k]; t += BT) s += v[t];
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) P.xx[k][0] = tot;
}

// Builds the padded off-diagonal copy of width S (pad_width, ipd_launch_plan.h; 0: none)
static void pad_flush(ipd_ctx* ctx, PadBatch* b) {
    if (b->n == 0) return;
    int rows = 1;
    for (int q = 0; q < b->n; ++q) rows = std::max(rows, b->N[q]);
    hipLaunchKernelGGL(k_pad_build_batch, dim3(std::max(1, std::min(cdiv(rows, 4), 4096)), b->n), dim3(256), 0,
                       ctx->stream, *b);
    IPD_KERNEL_CHECK();
    b->n = 0;
}
static void build_padded(ipd_ctx* ctx, Arena& ar, const Csr& A, int S, LevelDev* dev, PadBatch* batch) {
    dev->pci = nullptr;
    dev->pva = nullptr;
    dev->diag = nullptr;
    if (S == 0) return;
    unsigned short* pci = ar.alloc<unsigned short>((size_t)A.nr * S);
    double* pva = ar.alloc<double>((size_t)A.nr * S);
    double* diag = ar.alloc<double>((size_t)A.nr);
    {   // (launched with the other levels' copies: pad_flush)
        if (batch->n == PAD_BATCH) pad_flush(ctx, batch);
        const int q = batch->n++;
        batch->N[q] = A.nr;
        batch->S[q] = S;
        batch->rp[q] = A.rp;
        batch->ci[q] = A.ci;
        batch->va[q] = A.va;
        batch->pci[q] = pci;
        batch->pva[q] = pva;
        batch->diag[q] = diag;
    }
    dev->pci = pci;
    dev->pva = pva;
    dev->diag = diag;
}

// a batch of one (ipd_cycle_state.h)
void build_padded_private(ipd_amg* h, const Csr& A, int S, LevelDev* dev) {
    PadBatch one;
    build_padded(h->ctx, *h->arena, A, S, dev, &one);
    pad_flush(h->ctx, &one);
}

// The planners' switches, read at the call in which they take effect (amg_prepare_levels, amg_attach_maskop): the
// one place that reads them
PlanSwitches read_plan_switches() {
    PlanSwitches s;
    s.no_pad = switch_on("IPD_NO_PAD");
    s.no_stage = switch_on("IPD_NO_STAGE");
    s.no_rrc = switch_on("IPD_NO_RRC");
    s.no_poly = switch_on("IPD_NO_POLY");
    s.no_blk = switch_on("IPD_NO_BLK");
    s.no_bpoly = switch_on("IPD_NO_BPOLY");
    s.no_blkdense = switch_on("IPD_NO_BLKDENSE");
    s.no_small = switch_on("IPD_NO_SMALL");
    s.no_subcycle = switch_on("IPD_NO_SUBCYCLE");
    s.no_resident = switch_on("IPD_NO_RESIDENT");
    s.no_resident_remote = switch_on("IPD_NO_RESIDENT_REMOTE");
    s.no_resident_three = switch_on("IPD_NO_RESIDENT_THREE");
    s.no_resident_deep = switch_on("IPD_NO_RESIDENT_DEEP");
    s.no_resident_big = switch_on("IPD_NO_RESIDENT_BIG");
    s.no_res_poly4 = switch_on("IPD_NO_RES_POLY4");
    s.resident_big = switch_on("IPD_RESIDENT_BIG");
    s.maskop = switch_on("IPD_MASKOP");
    if (const char* e = switch_value("IPD_RESIDENT_G")) s.resident_g = std::atoi(e);
    if (const char* e = switch_value("IPD_RESIDENT_RANKS")) s.resident_ranks = std::atoi(e);
    if (const char* e = switch_value("IPD_RES_PRESLEEP")) s.res_presleep = std::max(0, std::atoi(e));
    if (const char* e = switch_value("IPD_RES_DEBUG_SKIP_PUBLISH")) s.res_skip_publish = (unsigned)std::max(0, std::atoi(e));
    s.res_no_full = switch_on("IPD_RES_NO_FULL");
    return s;
}

// the levels as the planners look at them (ipd_cycle_state.h)
std::vector<LevelShape> level_shapes(const ipd_amg* h, const CycleState* st) {
    std::vector<LevelShape> shapes((size_t)h->J + 1);
    for (int k = 1; k <= h->J; ++k) {
        const Level& lv = h->L[k];
        LevelShape& s = shapes[(size_t)k];
        s.nr = lv.A.nr;
        s.nnz = lv.A.nnz;
        s.nf = lv.nf;
        s.maxoff = st->run[(size_t)k].maxoff;
        s.p_nnz = k >= 2 ? lv.P.nnz : 0;
    }
    return shapes;
}

// launches the batch of levels and starts a new one (a hierarchy of more than PREP_ML levels takes several)
static void prep_flush(ipd_ctx* ctx, PrepLevels* p) {
    if (p->n == 0) return;
    hipLaunchKernelGGL(k_levels_prepare, dim3(p->first_block[p->n]), dim3(256), 0, ctx->stream, *p);
    IPD_KERNEL_CHECK();
    hipLaunchKernelGGL(k_levels_sum, dim3(p->n), dim3(BT), 0, ctx->stream, *p);
    IPD_KERNEL_CHECK();
    p->n = 0;
}
// Per-level vectors and constants (k_levels_prepare), the launch plan of every level and the padded copies
// it asks for: st->run[k].plan, st->run[k].dev
static void prepare_level_runs(ipd_amg* h, CycleState* st, const LaunchSwitches& sw) {
    ipd_ctx* ctx = h->ctx;
    Arena& ar = *h->arena;
    // first pass: per-level vectors and the longest off-diagonal row of every level (one
    // readback for all levels), then the launch plan, second pass: padded copies and launch geometry
    int* maxoff = zeroed<int>(ctx, (size_t)h->J + 1);
    // levels whose constant data come from the donor hierarchy (see ipd_amg::donor)
    const ipd_amg* donor = h->donor.get();
    const CycleState* dst_ = donor ? donor->cyc.get() : nullptr;
    auto shared_level = [&](int k) { return dst_ && k <= 2 && k <= donor->J; };
    PrepLevels prep;
    prep.n = 0;
    prep.first_block[0] = 0;
    for (int k = 1; k <= h->J; ++k) {
        Level& lv = h->L[k];
        const int N = lv.A.nr;
        lv.N = N;
        lv.nf = (k == 1 && h->opts.bigph) ? (int)h->opts.fnode : 0;
        IPD_REQUIRE(lv.nf < N, IPD_E_ARG, "fnode must be smaller than the matrix size");
        const Level* dl = shared_level(k) ? &donor->L[k] : nullptr;
        lv.dinv = dl ? dl->dinv : ar.alloc<double>((size_t)N);
        lv.Axi = dl ? dl->Axi : ar.alloc<double>((size_t)N);
        lv.xx = dl ? dl->xx : ar.alloc<double>(1);
        lv.r = ar.alloc<double>((size_t)N);
        lv.e = ar.alloc<double>((size_t)N);
        lv.e2 = ar.alloc<double>((size_t)N);
        lv.w = ar.alloc<double>((size_t)N);
        lv.rr = ar.alloc<double>((size_t)N);
        if (dl) continue;
        if (prep.n == PREP_ML) prep_flush(ctx, &prep);
        const int q = prep.n++;
        prep.N[q] = N;
        prep.nf[q] = lv.nf;
        prep.rp[q] = lv.A.rp;
        prep.ci[q] = lv.A.ci;
        prep.va[q] = lv.A.va;
        prep.dinv[q] = lv.dinv;
        prep.Axi[q] = lv.Axi;
        prep.xx[q] = lv.xx;
        prep.maxoff[q] = maxoff + k;
        prep.first_block[q + 1] = prep.first_block[q] + std::max(1, std::min(cdiv(N, 16), 4096));
    }
    prep_flush(ctx, &prep);
    std::vector<int> hmax((size_t)h->J + 1);
    ctx->fetch(maxoff, hmax.data(), (size_t)h->J + 1);
    std::vector<LaunchShape> shapes((size_t)h->J + 1);
    for (int k = 1; k <= h->J; ++k) {
        const Level& lv = h->L[k];
        LaunchShape& s = shapes[(size_t)k] = LaunchShape{lv.A.nr, lv.A.nnz, lv.nf, hmax[(size_t)k]};
        if (k == h->J) break;
        const Level& cl = h->L[k + 1];
        s.Pt = MatShape{cl.Pt.nr, cl.Pt.nc, cl.Pt.nnz};
        s.P = MatShape{cl.P.nr, cl.P.nc, cl.P.nnz};
        s.t1 = cl.T1.rp != nullptr;
        s.T1 = MatShape{cl.T1.nr, cl.T1.nc, cl.T1.nnz};
    }
    LaunchLevel dplan[3];   // the donor's records: its padded copy goes with its geometry
    int dlevels = 0;
    for (int k = 1; k <= 2 && shared_level(k); ++k) dplan[dlevels = k] = dst_->run[(size_t)k].plan;
    const std::vector<LaunchLevel> plan = plan_launches(shapes.data(), h->J, ctx->num_cu, sw, dplan, dlevels);
    PadBatch pads;   // the levels' padded copies: one launch after the loop
    for (int k = 1; k <= h->J; ++k) {
        Level& lv = h->L[k];
        LevelRun& rn = st->run[(size_t)k];
        rn.plan = plan[(size_t)k];
        rn.dev.N = lv.N;
        rn.dev.nf = lv.nf;
        rn.dev.S = rn.plan.S;
        rn.dev.L = rn.plan.L;
        rn.dev.G = rn.plan.G;
        rn.dev.rp = lv.A.rp;
        rn.dev.ci = lv.A.ci;
        rn.dev.va = lv.A.va;
        rn.dev.dinv = lv.dinv;
        rn.dev.Axi = lv.Axi;
        rn.dev.xx = lv.xx;
        rn.dev.r = lv.r;
        rn.dev.rr = lv.rr;
        if (shared_level(k)) {
            const LevelDev& dd = dst_->run[(size_t)k].dev;
            rn.dev.pci = dd.pci;
            rn.dev.pva = dd.pva;
            rn.dev.diag = dd.diag;
        } else {
            build_padded(ctx, ar, lv.A, rn.plan.S, &rn.dev, &pads);
            rn.maxoff = hmax[(size_t)k];
        }
    }
    pad_flush(ctx, &pads);
}

// Restriction / prolongation arguments of the launches, the coarsest level's PCG, the solve's vectors
static void prepare_transfers(ipd_amg* h, CycleState* st) {
    Arena& ar = *h->arena;
    auto xfer = [](const Csr& m, const XferPlan& xp, const double* x, double* y, int add) {
        // nrows, ncols, L, G, row0, row1, rp, ci, va, x, y, add, staged
        return XferArgs{m.nr, m.nc, xp.L, xp.G, 0, m.nr, m.rp, m.ci, m.va, x, y, add, xp.staged ? 1 : 0};
    };
    for (int k = 1; k < h->J; ++k) {
        Level& fine = h->L[k];
        Level& coarse = h->L[k + 1];
        LevelRun& rn = st->run[(size_t)k];
        // restriction: rows of P' (coarse rows), gathers the fine residual
        rn.restrict_args = xfer(coarse.Pt, rn.plan.rest, fine.rr, coarse.r, 0);
        // prolongation: rows of P (fine rows), gathers the coarse correction
        rn.prolong_args = xfer(coarse.P, rn.plan.prol, coarse.e, fine.e, 1);
    }
    {   // coarsest level: PCG(A,r) with the 2-argument defaults (PCG.m:18-23)
        Level& cl = h->L[h->J];
        PcgArgs a;
        a.N = cl.A.nr;
        a.L = st->run[(size_t)h->J].plan.pcg_L;
        a.rp = cl.A.rp;
        a.ci = cl.A.ci;
        a.va = cl.A.va;
        a.rhs = cl.r;
        a.guess = nullptr;
        a.d = cl.e;
        a.work = ar.alloc<double>(4 * (size_t)cl.A.nr);
        a.tol = 1e-11;
        a.maxit = h->opts.pcg_maxit;
        a.precd = 2;
        a.out = nullptr;
        a.nresk = 0;
        st->run[(size_t)h->J].pcg = a;
    }
    st->num_cu = h->ctx->num_cu;
    st->hist = ar.alloc<double>(8);
    st->x2 = ar.alloc<double>((size_t)h->L[1].A.nr);
    h->x = ar.alloc<double>((size_t)h->L[1].A.nr);
    h->b = ar.alloc<double>((size_t)h->L[1].A.nr);
}

static const char* const IMAGE_ROLE_NAMES[] = {"solve", "sub", "sub3", "sub4", "none"};

void amg_prepare_levels(ipd_amg* h) {
    std::unique_ptr<CycleState> st(new CycleState());
    st->run.resize((size_t)h->J + 1);
    const PlanSwitches sw = read_plan_switches();
    prepare_level_runs(h, st.get(), sw);
    prepare_transfers(h, st.get());
    // single-workgroup kernels: which levels, in which form, in which LDS images (ipd_level_plan.h)
    const std::vector<LevelShape> shapes = level_shapes(h, st.get());
    PlanOptions po;
    po.cycle = h->opts.cycle;
    po.smoth = h->opts.smoth;
    po.twogrid = h->opts.twogrid;
    po.concurrent_pair = h->opts.concurrent_pair;
    const LevelPlan plan = plan_levels(shapes.data(), h->J, po, sw);
    const bool debug = switch_on("IPD_DEBUG_LEVELS");
    if (debug)
        for (int k = 1; k <= h->J; ++k)
            std::fprintf(stderr, "[ipd] launch plan: %s\n", launch_plan_line(st->run[(size_t)k].plan, k, h->J).c_str());
    if (debug)
        for (const ImageSpec& s : plan.images)
            std::fprintf(stderr, "[ipd] image %s: k_lds=%d k_semi=%d k_tiny=%d k_blk=%d stage=%zu lds=%zu%s\n",
                         IMAGE_ROLE_NAMES[s.role], s.k_lds, s.k_semi, s.k_tiny, s.k_blk, s.stage_bytes, s.lds,
                         plan.sub5 == s.role ? " (level-5 tail)" : "");
    ipd_ctx* ctx = h->ctx;
    optin_small_kernels(ctx);
    st->k_sub = plan.k_sub;
    st->sub_semi_root = plan.sub_semi_root;
    for (const ImageSpec& s : plan.images) pack_image(ctx, h, st.get(), shapes, plan, s);
    if (plan.small_ok) {
        st->solve_out = h->arena->alloc<double>(4 + 2 * ((size_t)std::max(h->opts.maxit, 0) + 2));
        st->small_ok = true;
    }
    st->sub5 = plan.sub5;
    prepare_resident(h, st.get(), shapes, sw);
    if (debug) {
        std::fprintf(stderr, "[ipd] J=%d small=%d k_sub=%d ", h->J, (int)st->small_ok, st->k_sub);
        print_resident_summary(stderr, st.get());
        std::fprintf(stderr, " levels:");
        for (int k = 1; k <= h->J; ++k) std::fprintf(stderr, " %d/%d", h->L[k].A.nr, h->L[k].A.nnz);
        std::fprintf(stderr, "\n");
    }
    h->cyc = std::shared_ptr<CycleState>(st.release());
}

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
// ---- fused-program emitter (which phases are queued: phase_is_small, ipd_launch_plan.h) -------
void flush_fused(ipd_ctx* ctx, CycleState* st) {
    if (st->pending.n == 0) return;
    hipLaunchKernelGGL(k_fused, dim3(1), dim3(BT), st->pending_lds, ctx->stream, st->pending);
    IPD_KERNEL_CHECK();
    st->pending.n = 0;
    st->pending_lds = 0;
}

static PhaseDesc& push_phase(ipd_ctx* ctx, CycleState* st, int type, int stage_len) {
    if (st->pending.n == FUSED_MAX) flush_fused(ctx, st);
    PhaseDesc& d = st->pending.d[st->pending.n++];
    d.type = type;
    d.pad_ = 0;
    st->pending_lds = std::max(st->pending_lds, sizeof(double) * (size_t)stage_len);
    return d;
}

// Runs `launch(r0, r1, grid)` over the row range `rg` of a matrix walked by L lanes per row.  Unsharded: one
// call with the planned grid.  Sharded: this rank's slice only (its grid: the slice's own), followed by one
// grouped RCCL all-gather of the vectors the launch produced (each rank wrote its own slice of every one of them).
template <class F>
static void run_rows(ipd_ctx* ctx, CycleState* st, const RowRange& rg, int L, F launch,
                     std::initializer_list<double*> produced) {
    flush_fused(ctx, st);  // big launch: everything queued before it must run first
    const int G = st->shard_ranks;
    const int lo = rg.r0, rows = rg.r1 - rg.r0;
    if (G <= 1 || rows % G != 0 || rows < st->shard_min_rows) {  // replicated level
        launch(rg.r0, rg.r1, rg.G);
        return;
    }
    const int cnt = rows / G, grid = pick_blocks(cnt, L, st->num_cu);
    if (st->shard_emulate) {
        for (int vr = 0; vr < G; ++vr) launch(lo + vr * cnt, lo + (vr + 1) * cnt, grid);
        return;
    }
    launch(lo + st->shard_rank * cnt, lo + (st->shard_rank + 1) * cnt, grid);
    double* bases[4];
    int nv = 0;
    for (double* v : produced)
        if (v) bases[nv++] = v + lo;
    comm_allgather_inplace(ctx, bases, nv, cnt);
}

static void launch_smooth(ipd_ctx* ctx, const SmoothArgs& a, int grid) {
    const size_t dyn = a.staged ? sizeof(double) * (size_t)a.lv.N : 0;
    dispatch_staged_pad(a.staged, a.lv.S > 0, [&](auto S, auto P) {
        hipLaunchKernelGGL((k_smooth<decltype(S)::value, decltype(P)::value>), dim3(grid), dim3(BT), decltype(S)::value ? dyn : 0, ctx->stream, a);
    });
    IPD_KERNEL_CHECK();
}

// a restriction or prolongation as planned: queued into the fused program or launched over its rows
static void issue_xfer(ipd_ctx* ctx, CycleState* st, XferArgs a, const XferPlan& xp) {
    if (xp.queued) {
        push_phase(ctx, st, PH_XFER, a.ncols).u.x = a;
        return;
    }
    const size_t dyn = a.staged ? sizeof(double) * (size_t)a.ncols : 0;
    run_rows(ctx, st, RowRange{0, a.nrows, xp.G}, a.L,
             [&](int r0, int r1, int grid) {
                 a.row0 = r0;
                 a.row1 = r1;
                 if (a.staged)
                     hipLaunchKernelGGL(k_xfer<true>, dim3(grid), dim3(BT), dyn, ctx->stream, a);
                 else
                     hipLaunchKernelGGL(k_xfer<false>, dim3(grid), dim3(BT), 0, ctx->stream, a);
                 IPD_KERNEL_CHECK();
             },
             {a.y});
}

static void launch_resid(ipd_ctx* ctx, const LevelRun& rn, const double* e, int r0, int r1,
                         int grid) {
    const size_t dyn = rn.plan.staged ? sizeof(double) * (size_t)rn.dev.N : 0;
    dispatch_staged_pad(rn.plan.staged, rn.dev.S > 0, [&](auto S, auto P) {
        hipLaunchKernelGGL((k_resid<decltype(S)::value, decltype(P)::value>), dim3(grid), dim3(BT), decltype(S)::value ? dyn : 0, ctx->stream, rn.dev, e, r0, r1);
    });
    IPD_KERNEL_CHECK();
}

// one smoother sweep on level k: Jacobi = one launch, bigraph GS = two half launches
void launch_sweep(ipd_amg* h, CycleState* st, int k, int isnsp, bool post) {
    ipd_ctx* ctx = h->ctx;
    Level& lv = h->L[k];
    LevelRun& rn = st->run[(size_t)k];
    SmoothArgs a;
    a.lv = rn.dev;
    a.eold = lv.e;
    a.enew = lv.e2;
    a.win = lv.w;
    a.wout = lv.w;
    a.isnsp = isnsp;
    a.staged = rn.plan.staged;
    a.eold_zero = rn.e_zero ? 1 : 0;
    const LaunchLevel& p = rn.plan;
    // How a range is issued: queued into the fused program (replicated on every rank), or as launches of the
    // bit-mask kernel (level 1 with a mask operator: same two half sweeps, 1 bit per matrix entry; sharded runs
    // give each owner its block of the half's rows -- a row range inside one half is all the kernel needs) or
    // of the rows kernel
    const bool mask = k == 1 && lv.nf > 0 && st->mask_ok;
    const MaskOp& mo = st->maskop;
    auto rows = [&](int r0, int r1, int grid) {
        a.row0 = r0;
        a.row1 = r1;
        if (p.sweep_queued) {
            push_phase(ctx, st, PH_SMOOTH, lv.N).u.s = a;
        } else if (!mask) {
            launch_smooth(ctx, a, grid);
        } else {
            const size_t dyn = sizeof(double) * 64 * (size_t)std::max(mo.nwf, mo.nwc);
            const int nwh = (r0 < mo.nf) ? mo.nwf : mo.nwc;
            const int mgrid = std::max(1, cdiv(r1 - r0, std::min(MASK_RW, 64 / nwh) * (BT / 64)));
            hipLaunchKernelGGL(k_smooth_mask, dim3(mgrid), dim3(BT), dyn, ctx->stream, a, mo);
            IPD_KERNEL_CHECK();
        }
    };
    // Jacobi: one range.  Bigraph GS: the first half hands its result (wout) to the second, which updates with it
    const HalfRanges& hr = p.sweep[post ? 1 : 0];
    a.u0 = a.u1 = 0;
    for (int i = 0; i < hr.n; ++i) {
        if (i == hr.n - 1) a.wout = nullptr;
        if (p.sweep_queued)
            rows(hr.r[i].r0, hr.r[i].r1, 0);
        else
            run_rows(ctx, st, hr.r[i], a.lv.L, rows, {a.enew, a.wout});
        a.u0 = hr.r[i].r0;
        a.u1 = hr.r[i].r1;
    }
    rn.e_zero = false;
    std::swap(lv.e, lv.e2);
}

// (ipd_cycle_state.h)
bool build_maskop(ipd_amg* h, const double* p_dev, const double* q_dev, int m, int n, double tk, int* bad, MaskOp* out) {
    ipd_ctx* ctx = h->ctx;
    const Level& lv = h->L[1];
    Arena& ar = *h->arena;
    MaskOp mo;
    mo.nf = n;
    mo.nc = m;
    mo.nwf = cdiv(m, 64);
    mo.nwc = cdiv(n, 64);
    unsigned long long* fb = ar.alloc<unsigned long long>((size_t)n * mo.nwf);
    unsigned long long* cb = ar.alloc<unsigned long long>((size_t)m * mo.nwc);
    double* alpha = ar.alloc<double>((size_t)n);
    double* beta = ar.alloc<double>((size_t)m);
    double* diag = ar.alloc<double>((size_t)lv.N);
    IPD_HIP(hipMemsetAsync(fb, 0, sizeof(unsigned long long) * (size_t)n * mo.nwf, ctx->stream));
    IPD_HIP(hipMemsetAsync(cb, 0, sizeof(unsigned long long) * (size_t)m * mo.nwc, ctx->stream));
    IPD_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_maskop_scales, dim3(cdiv(lv.N, 256)), dim3(256), 0, ctx->stream, n, m, p_dev,
                       q_dev, 1.0 / tk, alpha, beta);
    hipLaunchKernelGGL(k_maskop_build, dim3(std::max(1, std::min(cdiv(lv.N, 4), 2048))), dim3(256), 0,
                       ctx->stream, lv.N, n, lv.A.rp, lv.A.ci, lv.A.va, (const double*)alpha,
                       (const double*)beta, mo.nwf, mo.nwc, fb, cb, diag, bad);
    IPD_KERNEL_CHECK();
    if (ctx->fetch1(bad) != 0) return false;
    mo.fbits = fb;
    mo.cbits = cb;
    mo.alpha = alpha;
    mo.beta = beta;
    mo.diag = diag;
    *out = mo;
    return true;
}

// Solves A_k e = r_k approximately; r in L[k].r, result in L[k].e.
// keep_e: start from the current L[k].e (second leg of a W cycle); otherwise the
// start is e = 0, which is never materialised (the first sweep does not read it).
void amg_cycle(ipd_amg* h, int k, int isnsp, bool wcycle, bool keep_e) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    Level& lv = h->L[k];
    LevelRun& rn = st->run[(size_t)k];
    const LaunchLevel& p = rn.plan;
    if (st->k_sub == k) {  // everything from here down: one workgroup, LDS-resident (replicated)
        flush_fused(ctx, st);
        launch_subcycle(ctx, st, keep_e);
        rn.e_zero = false;
        return;
    }
    if (k == h->J) {                                   // MG_Vcycle.m:43 / MG_Wcycle.m:44
        PcgArgs a = rn.pcg;                            // replicated on every rank
        a.rhs = lv.r;
        a.d = lv.e;
        push_phase(ctx, st, PH_PCG, 0).u.p = a;
        return;
    }
    const int nu = h->opts.smoth;
    if (!keep_e) {
        rn.e_zero = true;
        if (nu == 0) {  // no sweep will overwrite the iterate: materialise the zero
            flush_fused(ctx, st);
            IPD_HIP(hipMemsetAsync(lv.e, 0, sizeof(double) * (size_t)lv.N, ctx->stream));
            rn.e_zero = false;
        }
    }
    for (int s = 0; s < nu; ++s) launch_sweep(h, st, k, isnsp, false);          // :14-25
    XferArgs ra = rn.restrict_args;
    if (p.rrc) {
        // r_{k+1} = P'r - (P'A) e: one launch instead of residual + restriction           :27
        const Csr& T1 = h->L[k + 1].T1;
        RrcArgs rc;
        rc.p = ra;
        rc.p.x = lv.r;
        rc.p.L = p.rrc_walk.L;
        rc.rp2 = T1.rp;
        rc.ci2 = T1.ci;
        rc.va2 = T1.va;
        rc.e = lv.e;
        const bool staged = p.rrc_walk.staged;
        const size_t dyn = staged ? 2 * sizeof(double) * (size_t)ra.ncols : 0;
        run_rows(ctx, st, RowRange{0, ra.nrows, p.rrc_walk.G}, rc.p.L,
                 [&](int r0, int r1, int grid) {
                     rc.p.row0 = r0;
                     rc.p.row1 = r1;
                     if (staged)
                         hipLaunchKernelGGL(k_rrc<true>, dim3(grid), dim3(BT), dyn, ctx->stream, rc);
                     else
                         hipLaunchKernelGGL(k_rrc<false>, dim3(grid), dim3(BT), 0, ctx->stream, rc);
                     IPD_KERNEL_CHECK();
                 },
                 {ra.y});
    } else {
        if (p.resid_queued) {                                                           // :27
            ResidDesc& rd = push_phase(ctx, st, PH_RESID, lv.N).u.r;
            rd.lv = rn.dev;
            rd.e = lv.e;
            rd.row0 = 0;
            rd.row1 = lv.N;
        } else {
            run_rows(ctx, st, RowRange{0, lv.N, p.G_all}, rn.dev.L,
                     [&](int r0, int r1, int grid) { launch_resid(ctx, rn, lv.e, r0, r1, grid); }, {lv.rr});
        }
        issue_xfer(ctx, st, ra, p.rest);
    }
    amg_cycle(h, k + 1, isnsp, wcycle, false);                                   // :29
    // MG_Wcycle.m:30 -- the second correction; on the coarsest level it repeats the
    // identical zero-guess PCG solve, so it is skipped there (same bits).
    if (wcycle && k + 1 < h->J) amg_cycle(h, k + 1, isnsp, wcycle, true);
    XferArgs pa = rn.prolong_args;                                               // :31
    pa.x = h->L[k + 1].e;
    pa.y = lv.e;
    issue_xfer(ctx, st, pa, p.prol);
    for (int s = 0; s < nu; ++s) launch_sweep(h, st, k, isnsp, true);           // :33-41
}

void launch_top(ipd_amg* h, CycleState* st, const double* b, const double* x,
                       const double* e, double* xnew, bool first) {
    ipd_ctx* ctx = h->ctx;
    LevelRun& rn = st->run[1];
    TopArgs a;
    a.lv = rn.dev;
    a.b = b;
    a.x = x;
    a.e = e;
    a.xnew = xnew;
    a.staged = rn.plan.staged;
    const size_t dyn = a.staged ? sizeof(double) * (size_t)rn.dev.N : 0;
    if (rn.plan.top_queued) {
        a.row0 = 0;
        a.row1 = rn.dev.N;
        push_phase(ctx, st, PH_TOP, rn.dev.N).u.t = a;
    } else {
        run_rows(ctx, st, RowRange{0, rn.dev.N, rn.plan.G_all}, rn.dev.L,
                 [&](int r0, int r1, int grid) {
                     a.row0 = r0;
                     a.row1 = r1;
                     dispatch_staged_pad(a.staged, rn.dev.S > 0, [&](auto S, auto P) {
                         hipLaunchKernelGGL((k_top<decltype(S)::value, decltype(P)::value>), dim3(grid), dim3(BT), decltype(S)::value ? dyn : 0, ctx->stream, a);
                     });
                     IPD_KERNEL_CHECK();
                 },
                 {rn.dev.r, xnew});
    }
    ConvArgs ca;
    ca.r = rn.dev.r;
    ca.n = rn.dev.N;
    ca.hist = st->hist;
    ca.first = first ? 1 : 0;
    push_phase(ctx, st, PH_CONV, 0).u.c = ca;
    flush_fused(ctx, st);  // the loop body ends here: nothing stays queued across calls
}

// one Class_AMG loop body (Class_AMG.m:96-105): x_out = x_in + cycle(b - A x_in)
void enqueue_loop_body(ipd_amg* h, CycleState* st, const double* b, const double* xin,
                              double* xout) {
    const bool wc = h->opts.cycle == 'w', vc = h->opts.cycle == 'v';
    const double* ecorr = nullptr;
    if (vc || wc) {
        amg_cycle(h, 1, h->opts.isnsp, wc, false);
        ecorr = h->L[1].e;
    }
    launch_top(h, st, b, xin, ecorr, xout, false);
}

static void copy_vec(ipd_ctx* ctx, double* dst, const double* src, int N) {
    IPD_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
}

// x = the initial guess (NULL: zeros)
static void load_guess(ipd_ctx* ctx, double* x, const double* guess_dev, int N) {
    if (guess_dev)
        copy_vec(ctx, x, guess_dev, N);
    else
        IPD_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)N, ctx->stream));
}

// Class_AMG.m:86-109
void amg_solve_dev(ipd_amg* h, const double* b_dev, const double* guess_dev, double* x_dev,
                   int32_t* it_out, double* rel_res_out, double* rel_resk, double* rhok) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    const AmgOpts& o = h->opts;
    const int N = h->L[1].A.nr;
    double* xa = h->x;
    double* xb = st->x2;
    load_guess(ctx, xa, guess_dev, N);
    // what a one-launch solve read back: iterations, last relative residual, then the two histories
    auto deliver = [&](const std::vector<double>& out) {
        const int its = (int)out[0];
        if (rel_resk) std::memcpy(rel_resk, out.data() + 4, sizeof(double) * ((size_t)its + 1));
        if (rhok) std::memcpy(rhok, out.data() + 4 + (o.maxit + 2), sizeof(double) * ((size_t)its + 1));
        if (x_dev) copy_vec(ctx, x_dev, xa, N);
        if (it_out) *it_out = its;
        if (rel_res_out) *rel_res_out = out[1];
        ctx->sync();
    };
    if (st->small_ok && st->shard_ranks == 1) {
        // small hierarchy: the whole solve phase is one single-workgroup launch
        launch_solve_small(ctx, st, b_dev, xa, 0);
        const size_t nout = 4 + 2 * ((size_t)o.maxit + 2);
        std::vector<double> out(nout);
        ctx->fetch(st->solve_out, out.data(), nout);
        deliver(out);
        return;
    }
    if (resident_active(st) && st->shard_ranks == 1) {
        // dense regime: the whole solve phase is one launch of co-resident workgroups
        std::vector<double> out;
        if (run_resident(h, st, b_dev, xa, 0, &out, nullptr)) {
            deliver(out);
            return;
        }
        // not usable right now: restore the initial guess and take the multi-launch path
        load_guess(ctx, xa, guess_dev, N);
    }
    launch_top(h, st, b_dev, xa, nullptr, xb, true);                            // :89
    std::swap(xa, xb);
    double hh[5];
    ctx->fetch(st->hist, hh, 5);
    int it = 0;
    double rel_res = 0.0;
    if (hh[0] == 0.0) {                                                          // :91-92
        if (rel_resk) rel_resk[0] = 0.0;
        if (rhok) rhok[0] = INFINITY;
    } else {
        it = 1;                                                                  // :94
        double last_rel = 1.0;
        if (rel_resk) rel_resk[0] = 1.0;
        if (rhok) rhok[0] = NAN;
        while (last_rel > o.retol && it <= o.maxit) {                            // :95
            enqueue_loop_body(h, st, b_dev, xa, xb);                             // :96-105
            std::swap(xa, xb);
            ctx->fetch(st->hist, hh, 5);
            rel_res = hh[3];
            last_rel = rel_res;
            if (rel_resk) rel_resk[it] = rel_res;
            if (rhok) rhok[it] = hh[4];
            ++it;
            if (hh[4] > 1.0) break;                                              // :106
        }
        it -= 1;                                                                 // :108
    }
    if (x_dev) copy_vec(ctx, x_dev, xa, N);
    if (xa != h->x) std::swap(h->x, st->x2);  // keep h->x pointing at the current iterate
    if (it_out) *it_out = it;
    if (rel_res_out) *rel_res_out = rel_res;
    ctx->sync();
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_amg_solve_dev(ipd_amg* h, const double* b_dev, const double* guess_dev,
                                 double* x_dev, int32_t* it, double* rel_res, double* rel_resk,
                                 double* rhok) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b_dev && x_dev, IPD_E_ARG, "NULL argument");
        CallScope scope(h->ctx);
        amg_solve_dev(h, b_dev, guess_dev, x_dev, it, rel_res, rel_resk, rhok);
    });
}

extern "C" int ipd_amg_solve(ipd_amg* h, const double* b, const double* guess, double* x,
                             int32_t* it, double* rel_res, double* rel_resk, double* rhok) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b && x, IPD_E_ARG, "NULL argument");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        const size_t N = (size_t)h->L[1].A.nr;
        double* db = ctx->scratch->alloc<double>(N);
        double* dg = nullptr;
        double* dx = ctx->scratch->alloc<double>(N);
        ctx->upload(db, b, N);
        if (guess) {
            dg = ctx->scratch->alloc<double>(N);
            ctx->upload(dg, guess, N);
        }
        amg_solve_dev(h, db, dg, dx, it, rel_res, rel_resk, rhok);
        ctx->fetch(dx, x, N);
    });
}

static void run_cycle_api(ipd_amg* h, const double* r, int isnsp, int k, const double* e_in,
                          double* e_out, bool wc) {
    IPD_REQUIRE(h && r && e_out, IPD_E_ARG, "NULL argument");
    IPD_REQUIRE(k >= 1 && k <= h->J, IPD_E_ARG, "level k out of range");
    ipd_ctx* ctx = h->ctx;
    CallScope scope(ctx);
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    Level& lv = h->L[k];
    const size_t N = (size_t)lv.A.nr;
    ctx->upload(lv.r, r, N);
    LevelRun& rn = st->run[(size_t)k];
    bool keep = false;
    if (e_in && wc) {  // MG_Wcycle(r,isnsp,k,e): start from the caller's iterate
        ctx->upload(lv.e, e_in, N);
        rn.e_zero = false;
        keep = true;
    }
    amg_cycle(h, k, isnsp, wc, keep);
    flush_fused(ctx, st);
    ctx->fetch(h->L[k].e, e_out, N);
}

// ---- the cycle as a preconditioner (ipd_krylov.hip) -------------------------------------
bool amg_level1_walk(ipd_amg* h, LevelDev* lv, int* staged, int* grid) {
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    if (st->shard_ranks > 1 && !st->shard_emulate) return false;
    const LevelRun& rn = st->run[1];
    *lv = rn.dev;
    *staged = rn.plan.staged ? 1 : 0;
    *grid = rn.plan.G_all;
    return true;
}

// ---- the launch-path cycle's CSR forms, for the block solve (ipd_block.hip) ----------------
bool amg_block_levels(ipd_amg* h, std::vector<BlockLevel>* out) {
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    if (st->shard_ranks > 1) return false;
    if (!out) return true;
    auto csr_of = [](const Csr& m, int L, int grid) { return BlockCsr{m.nr, m.nc, L, grid, m.rp, m.ci, m.va}; };
    out->assign((size_t)h->J + 1, BlockLevel{});
    for (int k = 1; k <= h->J; ++k) {
        const Level& lv = h->L[k];
        const LevelRun& rn = st->run[(size_t)k];
        BlockLevel& bl = (*out)[(size_t)k];
        bl.N = lv.N;
        bl.nf = lv.nf;
        const LaunchLevel& p = rn.plan;
        bl.A = csr_of(lv.A, p.L, p.G_all);
        bl.sweep[0] = p.sweep[0];
        bl.sweep[1] = p.sweep[1];
        bl.dinv = lv.dinv;
        bl.Axi = lv.Axi;
        bl.xx = lv.xx;
        if (k < h->J) {
            const Level& cl = h->L[k + 1];
            bl.Pt = csr_of(cl.Pt, p.rest.L, p.rest.G);
            bl.P = csr_of(cl.P, p.prol.L, p.prol.G);
            if (p.rrc_rule) bl.T1 = csr_of(cl.T1, p.rrc_walk.L, p.rrc_walk.G);
        } else {
            const PcgArgs& a = rn.pcg;
            bl.pcg_L = a.L;
            bl.pcg_precd = a.precd;
            bl.pcg_tol = a.tol;
            bl.pcg_maxit = a.maxit;
        }
    }
    return true;
}

void amg_apply_cycle(ipd_amg* h) {
    const int cyc = h->opts.cycle;
    IPD_REQUIRE(cyc == 'v' || cyc == 'w', IPD_E_ARG, "AMG-PCG: the hierarchy's cycle must be 'v' or 'w'");
    amg_cycle(h, 1, h->opts.isnsp, cyc == 'w', false);   // what run_cycle_api(h, r, isnsp, 1, NULL, ..) runs
    flush_fused(h->ctx, state_of(h));
}

extern "C" int ipd_amg_vcycle(ipd_amg* h, const double* r, int isnsp, int k, double* e) {
    return ipd_guard([&] { run_cycle_api(h, r, isnsp, k, nullptr, e, false); });
}

extern "C" int ipd_amg_wcycle(ipd_amg* h, const double* r, int isnsp, int k, const double* e_in,
                              double* e_out) {
    return ipd_guard([&] { run_cycle_api(h, r, isnsp, k, e_in, e_out, true); });
}

extern "C" int ipd_class_amg(ipd_ctx* ctx, const ipd_csc* A, const double* b, const double* guess,
                             const ipd_amg_opts* o, ipd_rng* rng, double* x, int32_t* it,
                             double* rel_res, double* rel_resk, double* rhok) {
    ipd_amg* h = nullptr;
    int rc = ipd_amg_setup(ctx, A, o, rng, &h);
    if (rc != IPD_OK) return rc;
    rc = ipd_amg_solve(h, b, guess, x, it, rel_res, rel_resk, rhok);
    ipd_amg_destroy(h);
    return rc;
}

extern "C" int ipd_pcg(ipd_ctx* ctx, const ipd_csc* H, const double* e, const double* guess,
                       const ipd_pcg_opts* o, double* d, int64_t* it, double* res, double* resk) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && H && e && d, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        Arena& tmp = *ctx->scratch;
        double tol = 1e-11;
        long long maxit = 10000;
        int precd = 2;  // PCG.m:24-27 defaults
        long long nf = 0;
        if (o) {
            if (o->retol >= 0) tol = o->retol;
            if (o->maxit >= 0) maxit = o->maxit;
            if (o->precd >= 0) precd = o->precd;
            nf = o->nf;
        }
        Csr hm;
        csr_upload_from_csc(ctx, tmp, H, false, &hm);  // true rows of H
        const size_t N = (size_t)hm.nr;
        double* de = tmp.alloc<double>(N);
        double* dd = tmp.alloc<double>(N);
        double* dg = nullptr;
        ctx->upload(de, e, N);
        if (guess) {
            dg = tmp.alloc<double>(N);
            ctx->upload(dg, guess, N);
        }
        long long its = 0;
        pcg_dev(ctx, hm, de, dg, tol, maxit, precd, dd, &its, res, resk, nf);
        if (it) *it = its;
        ctx->fetch(dd, d, N);
    });
}
