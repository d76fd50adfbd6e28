// The single-workgroup interpreter of the cycle (device only): one workgroup runs the V/W recursion itself
// (MG_Vcycle.m:12-45, MG_Wcycle.m:13-46) on the levels of a SolveDesc, most of them cached in an LDS image
// (ipd_level_plan.h lays it out, pack_image packs it).  k_solve_small, k_pcg_small and k_subcycle (ipd_cycle.hip)
// and the tail workgroup of the resident kernels (ipd_resident_proto.h) are its callers; every function is
// inlined into them.
#pragma once

#include "ipd_cycle_args.h"
#include "ipd_cycle_pcg.h"

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
// The context a workgroup starts with on descriptor D: staging area at the head of its dynamic LDS, every iterate
// in its own array, none known to be zero, no operator copy loaded.  blkpart: 48 + SOLVE_ML + 1 doubles.
__device__ __forceinline__ SolveCtx sol_ctx(const SolveDesc* D, PhaseLds* lds, double* red, double* blkpart,
                                            char* dyn_raw, long long* dbg) {
    SolveCtx c;
    c.D = D;
    c.lds = lds;
    c.red = red;
    c.xs = reinterpret_cast<double*>(dyn_raw);
    c.swapmask = 0;
    c.zeromask = 0;
    c.part = blkpart;
    c.sumr = blkpart + 48;
    c.dbg = dbg;
    c.bm_lds = 0;
    return c;
}
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
