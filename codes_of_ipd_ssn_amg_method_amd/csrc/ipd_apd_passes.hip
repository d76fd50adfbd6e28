// The mn-sized passes of one APD / semismooth-Newton iteration on device-resident vectors
// (SURVEY.md section 8 row f1): Class1/APD_SsN_Class1.m:101-275, Class2/APD_SsN_Class2.m:95-285.
//
// Every mn-sized vector (c, xk, vk, wk, phi, gama, the mask s) lives in HBM for the whole
// run; the host keeps only the scalars of the scripts (ak, bk, tk, norms, counters).
//
// The mn-sized work of one Newton step is ONE streaming pass (`OpEvalT`): from wk and the
// multiplier it forms zk = (wk - H'lk)/tk on the fly (never stored), writes the byte mask
// s = (0 <= zk <= gama), and reduces Ax(prox(zk)), |prox(zk)|^2, phi'prox(zk) -- i.e. Fk,
// the active set and the Armijo merit of one trial point come out of 8 bytes read + 1 byte
// written per entry, where the scripts make ~10 passes (Aty, zk, prox, Ax, norms, s).
// These passes are HBM-bound: 9 B/entry (class 1), 17 B/entry with phi (class 2).
//
// Each family is an op of the tile walker (ipd_apd_tiles.h), an epilogue kernel and the host function that
// launches both: begin, eval, merit, end.
#pragma clang fp contract(off)

#include <cmath>

#include "ipd_apd_state.h"

namespace {

// --- APD_SsN_Class1.m:125 / Class2 :119  wk = -wc + bk*(uk+ak*vk)/ak^2 ; partials of H*uk
template <class CS>   // CS: CostStored or CostFree<D> (ipd_apd_tiles.h)
struct OpBeginT {
    static constexpr bool NEED_AX = true;
    // matrix-free: 8 columns of q and D coordinates are what the scalar registers hold
    static constexpr int FC = CS::FREE ? 8 : 16;
    Prob P;
    const double* u;
    const double* v;
    double* w;
    double ak, bk, ak2;
    [[no_unique_address]] CS cs;
    struct Raw {
        double c, u, v, phi;
    };
    struct RowC {
        typename CS::Row x;
    };
    struct ColC {
        double q;
        typename CS::Col y;
    };
    __device__ void row_const(RowC& rc, int i) const { cs.row(rc.x, i); }
    __device__ void col_const(ColC& c, int j) const {
        c.q = P.q[j];
        cs.col(c.y, j);
    }
    __device__ void fetch(Raw& r, size_t idx) const {
        r.c = CS::FREE ? 0.0 : P.c[idx];
        r.u = u[idx];
        r.v = v[idx];
        r.phi = P.cls2 ? P.phi[idx] : 0.0;
    }
    __device__ double compute(const Raw& r, const RowC& rc, const ColC& cc, size_t idx, double* sc) const {
        const double c = cs.value(r.c, rc.x, cc.y);
        w[idx] = -c + bk * (r.u + ak * r.v) / ak2;
        sc[3] += r.phi * r.u;
        return r.u;
    }
};

// --- :139-144,182-196  zk, s, prox(zk) and its reductions at one multiplier.
// Compile-time variants (class 2 / vector gama / the prob-3 merit): the pass is HBM-bound only
// if the per-entry state stays small -- a runtime-flagged version kept 48 loads and three extra
// accumulators alive per lane and ran at a third of the bandwidth.
template <bool CLS2, bool GVEC, bool M3>
struct OpEvalT {
    static constexpr bool NEED_AX = true;
    static constexpr int FC = 16;
    Prob P;
    const double* w;
    uint8_t* s;
    Lam lam;
    double itk;  // 1/tk
    struct Raw {
        double w, phi, g;
    };
    struct RowC {
        double pi, y2, lamL;
    };
    struct ColC {
        double y1, q;
    };
    __device__ void row_const(RowC& rc, int i) const {
        rc.pi = P.p[i];
        rc.y2 = lam.at(P.n + i);
        rc.lamL = CLS2 ? lam.at(P.m + P.n) : 0.0;
    }
    __device__ void col_const(ColC& c, int j) const {
        c.y1 = lam.at(j);
        c.q = P.q[j];
    }
    __device__ void fetch(Raw& r, size_t idx) const {
        r.w = w[idx];
        if (CLS2) r.phi = P.phi[idx];
        if (GVEC) r.g = P.gama[idx];
    }
    __device__ double compute(const Raw& r, const RowC& rc, const ColC& cc, size_t idx,
                              double* sc) const {
        double aty = rc.pi * cc.y1 + rc.y2 * cc.q;                  // Aty.m:12-13
        if (CLS2) aty = aty + rc.lamL * r.phi;                      // Class2 :139
        const double z = itk * (r.w - aty);
        const double g = GVEC ? r.g : P.gs;
        const double t = z > 0.0 ? z : 0.0;
        const double px = CLS2 ? t : (t < g ? t : g);               // prox (Class1 :32, Class2 :29)
        const bool act = CLS2 ? (z >= 0.0) : (z >= 0.0 && z <= g);
        s[idx] = act ? 1 : 0;
        sc[0] += px * px;
        if (M3) {
            sc[1] += z * z;
            sc[2] += (z - px) * (z - px);
        }
        if (CLS2) sc[3] += r.phi * px;
        sc[4] += act ? 1.0 : 0.0;
        return px;
    }
};

// --- :199-207  |prox(zk)|^2 at MK trial multipliers lk_old + step[k]*zeta in one pass over wk.
// A rejected Armijo test is followed by dozens of further trials (delta = 0.9; measured mean 57
// when the first one fails): they only need the merit, not Fk or the mask, so MK of them share
// one read of wk.  Per trial the arithmetic is that of OpEval, operation for operation.
struct OpMerit {
    static constexpr bool NEED_AX = false;
    static constexpr int FC = 16;
    Prob P;
    const double* w;
    const double* lam;
    const double* zeta;
    double step[MK];
    double itk;
    struct Raw {
        double w, phi, g;
    };
    struct RowC {
        double pi, l2, z2;
    };
    struct ColC {
        double l1, z1, q;
    };
    __device__ void row_const(RowC& rc, int i) const {
        rc.pi = P.p[i];
        rc.l2 = lam[P.n + i];
        rc.z2 = zeta[P.n + i];
    }
    __device__ void col_const(ColC& c, int j) const {
        c.l1 = lam[j];
        c.z1 = zeta[j];
        c.q = P.q[j];
    }
    __device__ void fetch(Raw& r, size_t idx) const {
        r.w = w[idx];
        r.phi = P.cls2 ? P.phi[idx] : 0.0;
        r.g = P.gama ? P.gama[idx] : P.gs;
    }
    __device__ double compute(const Raw& r, const RowC& rc, const ColC& cc, size_t, double* sc) const {
        const double l1 = cc.l1, z1 = cc.z1, qj = cc.q;
        const int M = P.m + P.n;
        const double lL = P.cls2 ? lam[M] : 0.0, zL = P.cls2 ? zeta[M] : 0.0;
#pragma unroll
        for (int k = 0; k < MK; ++k) {
            double aty = rc.pi * (l1 + step[k] * z1) + (rc.l2 + step[k] * rc.z2) * qj;
            if (P.cls2) aty = aty + (lL + step[k] * zL) * r.phi;
            const double z = itk * (r.w - aty);
            const double px = prox_of(P, z, r.g);
            sc[k] += px * px;
        }
        return 0.0;
    }
};

// --- :239-242,253-254  uk1 = prox(zk), vk1, and the KKT residuals of (uk1, lk1)
template <bool FROM_W, class CS>
struct OpEndT {
    static constexpr bool NEED_AX = true;
    // matrix-free: 4 columns of y1, q and D coordinates (8 spilled up to 73 scalar registers)
    static constexpr int FC = CS::FREE ? 4 : 8;
    Prob P;
    const double* w;      // FROM_W
    const double* uold;   // FROM_W: current iterate ; else: the iterate to measure
    double* unew;         // FROM_W
    double* v;            // FROM_W
    Lam lam;
    double itk, ak;
    [[no_unique_address]] CS cs;
    struct Raw {
        double w, u, c, phi, g;
    };
    struct RowC {
        double pi, y2;
        typename CS::Row x;
    };
    struct ColC {
        double y1, q;
        typename CS::Col y;
    };
    __device__ void row_const(RowC& rc, int i) const {
        rc.pi = P.p[i];
        rc.y2 = lam.at(P.n + i);
        cs.row(rc.x, i);
    }
    __device__ void col_const(ColC& c, int j) const {
        c.y1 = lam.at(j);
        c.q = P.q[j];
        cs.col(c.y, j);
    }
    __device__ void fetch(Raw& r, size_t idx) const {
        r.w = FROM_W ? w[idx] : 0.0;
        r.u = uold[idx];
        r.c = CS::FREE ? 0.0 : P.c[idx];
        r.phi = P.cls2 ? P.phi[idx] : 0.0;
        r.g = P.gama ? P.gama[idx] : P.gs;
    }
    __device__ double compute(const Raw& r, const RowC& rc, const ColC& cc, size_t idx,
                              double* sc) const {
        double aty = rc.pi * cc.y1 + rc.y2 * cc.q;
        if (P.cls2) aty = aty + lam.at(P.m + P.n) * r.phi;
        double u1 = r.u;
        if (FROM_W) {
            const double z = itk * (r.w - aty);
            u1 = prox_of(P, z, r.g);
            unew[idx] = u1;
            v[idx] = u1 + (u1 - r.u) / ak;
        }
        const double c = cs.value(r.c, rc.x, cc.y);
        const double d = u1 - prox_of(P, u1 - c - aty, r.g);       // :242 / Class2 :227
        sc[0] += d * d;
        sc[1] += c * u1;
        sc[3] += r.phi * u1;
        return u1;
    }
};

// ---------------------------------------------------------------------------
// epilogues (one workgroup of 1024 threads)
// ---------------------------------------------------------------------------
struct BeginFin {
    Parts pt;
    Prob P;
    const double* u;
    const double* v;
    double* w;
    const double* lam;
    const double* b;
    double* wlk;
    double ak, bk, ak2, bk1, ibk, mu;
};

__global__ __launch_bounds__(BT) void k_begin_fin(const BeginFin a) {
    __shared__ double red[16];
    const int M = a.P.m + a.P.n;
    const size_t mn = (size_t)a.P.m * a.P.n;
    const double phix = a.P.cls2 ? scal_total(a.pt, 3, red) : 0.0;
    for (int t = threadIdx.x; t < M; t += BT) {
        double Hu = ax_entry(a.pt, t);
        if (a.P.cls2) {
            Hu = Hu + a.u[mn + t];                                         // Ax(xk)+[yk;zk]
            a.w[mn + t] = -0.0 + a.bk * (a.u[mn + t] + a.ak * a.v[mn + t]) / a.ak2;
        }
        a.wlk[t] = a.bk1 * (a.lam[t] - a.ibk * (Hu - a.b[t])) - a.b[t];   // :126 / Class2 :120
    }
    if (a.P.cls2 && threadIdx.x == 0)
        a.wlk[M] = a.bk1 * (a.lam[M] - a.ibk * (phix - a.b[M])) - a.b[M];
}

struct EvalFin {
    Parts pt;
    Prob P;
    const double* w;
    Lam lam;
    const double* wlk;
    const double* Fold;  // with lam.zeta: Fk_old for ress = |Fk_old'*zeta| (:198)
    double* lam_out;
    double* F;
    double* tmask;       // class 2: t = zk(mn+1:end) >= 0 as 0/1 doubles (diag of T)
    double bk1, itk;
    ApdScal* out;
    double* fpart;   // per-block partial sums of the epilogue
    int* counter;    // ticket of the epilogue blocks (0 between launches)
};

// The epilogue of the evaluation pass runs once per line-search trial, so it is spread over
// cdiv(L, 128) small workgroups (one entry of Fk per thread: its 64+ partial sums arrive in two
// round trips instead of one workgroup walking 0.5 MB -- measured 36 us -> see DESIGN.md);
// the last workgroup to finish (ticket) adds the per-block scalars in block order.
constexpr int EB = 128;
constexpr int NFS = 6;   // f2, l2, wl, fz, tp2, tz2

__device__ __forceinline__ double sum128(double v, double* red) {   // result in every thread
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1];
}
__device__ __forceinline__ double scal_total128(const Parts& pt, int slot, double* red) {
    double a = 0.0;
    for (int b = threadIdx.x; b < pt.nblk; b += EB) a += pt.spart[(size_t)b * NSC + slot];
    return sum128(a, red);
}

__global__ __launch_bounds__(EB) void k_eval_fin(const EvalFin a) {
    __shared__ double red[2];
    __shared__ int is_last;
    const int M = a.P.m + a.P.n;
    const size_t mn = (size_t)a.P.m * a.P.n;
    const int L = M + (a.P.cls2 ? 1 : 0);
    const int t = blockIdx.x * EB + threadIdx.x;
    // phi'*prox(zk) is needed by the one thread that owns the last entry of Fk (class 2)
    double phix = 0.0;
    if (a.P.cls2 && blockIdx.x == M / EB) phix = scal_total128(a.pt, 3, red);
    double f2 = 0.0, l2 = 0.0, wl = 0.0, fz = 0.0, tp2 = 0.0, tz2 = 0.0;
    if (t < L) {
        const double lt = a.lam.at(t);
        double Hp;
        if (t < M) {
            Hp = ax_entry(a.pt, t);
            if (a.P.cls2) {
                const double z = a.itk * (a.w[mn + t] - lt);               // Htlk tail = lk(1:m+n)
                const double pz = z > 0.0 ? z : 0.0;
                if (a.tmask) a.tmask[t] = z >= 0.0 ? 1.0 : 0.0;
                Hp = Hp + pz;                                              // Class2 :141
                tp2 = pz * pz;
                tz2 = z * z;
            }
        } else {
            Hp = phix;
        }
        const double f = a.bk1 * lt - Hp - a.wlk[t];                       // :144
        a.F[t] = f;
        if (a.lam_out) a.lam_out[t] = lt;
        f2 = f * f;
        l2 = lt * lt;
        wl = a.wlk[t] * lt;
        if (a.lam.zeta && a.Fold) fz = a.Fold[t] * a.lam.zeta[t];
    }
    double vals[NFS] = {f2, l2, wl, fz, tp2, tz2};
#pragma unroll
    for (int k = 0; k < NFS; ++k) {
        const double sk = sum128(vals[k], red);
        if (threadIdx.x == 0) a.fpart[(size_t)blockIdx.x * NFS + k] = sk;
    }
    __threadfence();
    if (threadIdx.x == 0) is_last = (atomicAdd(a.counter, 1) == (int)gridDim.x - 1);
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    const double prox2 = scal_total128(a.pt, 0, red);
    const double z2s = scal_total128(a.pt, 1, red);
    const double zmp2 = scal_total128(a.pt, 2, red);
    const double cnt = scal_total128(a.pt, 4, red);
    // the partials arrive in one burst (one thread walking them was a chain of dependent loads); they
    // are still added in block order
    __shared__ double fp_lds[4 * EB];
    const int nfp = (int)gridDim.x * NFS;
    for (int e = threadIdx.x; e < nfp && e < 4 * EB; e += EB) fp_lds[e] = a.fpart[e];
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[NFS];
        for (int k = 0; k < NFS; ++k) tot[k] = 0.0;
        for (unsigned b = 0; b < gridDim.x; ++b)
            for (int k = 0; k < NFS; ++k)
                tot[k] += ((int)(b * NFS + k) < 4 * EB) ? fp_lds[b * NFS + k] : a.fpart[(size_t)b * NFS + k];
        a.out->normF2 = tot[0];
        a.out->lam2 = tot[1];
        a.out->wlk_lam = tot[2];
        a.out->fold_zeta = tot[3];
        a.out->prox2 = prox2 + tot[4];
        a.out->z2 = z2s + tot[5];
        a.out->zmp2 = zmp2;  // tails: z - prox(z) = min(z,0); only class 1 (prob 3) uses it
        a.out->count = cnt;
        *a.counter = 0;
    }
}

struct EndFin {
    Parts pt;
    Prob P;
    int from_w;
    const double* w;
    const double* uold;
    double* unew;
    double* v;
    Lam lam;
    const double* b;
    double itk, ak;
    ApdScal* out;
};

__global__ __launch_bounds__(BT) void k_end_fin(const EndFin a) {
    __shared__ double red[16];
    const int M = a.P.m + a.P.n;
    const size_t mn = (size_t)a.P.m * a.P.n;
    const double kx2 = scal_total(a.pt, 0, red);
    const double fx = scal_total(a.pt, 1, red);
    const double phix = scal_total(a.pt, 3, red);
    double ky2 = 0.0, kz2 = 0.0, kl2 = 0.0;
    for (int t = threadIdx.x; t < M; t += BT) {
        double Hu = ax_entry(a.pt, t);
        if (a.P.cls2) {
            const double lt = a.lam.at(t);
            double u1 = a.uold[mn + t];
            if (a.from_w) {
                const double z = a.itk * (a.w[mn + t] - lt);
                const double pz = z > 0.0 ? z : 0.0;
                a.unew[mn + t] = pz;
                a.v[mn + t] = pz + (pz - u1) / a.ak;
                u1 = pz;
            }
            Hu = Hu + u1;
            const double sh = u1 - lt;
            const double d = u1 - (sh > 0.0 ? sh : 0.0);                   // Class2 :225-226
            if (t < a.P.n)
                ky2 += d * d;
            else
                kz2 += d * d;
        }
        const double e = Hu - a.b[t];
        kl2 += e * e;
    }
    ky2 = block_sum(ky2, red);
    kz2 = block_sum(kz2, red);
    kl2 = block_sum(kl2, red);
    if (threadIdx.x == 0) {
        if (a.P.cls2) {
            const double e = phix - a.b[M];
            kl2 += e * e;
        }
        a.out->kx2 = kx2;
        a.out->ky2 = ky2;
        a.out->kz2 = kz2;
        a.out->kl2 = kl2;
        a.out->fx = fx;
    }
}

struct MeritFin {
    Parts pt;
    Prob P;
    const double* w;
    const double* lam;
    const double* zeta;
    const double* wlk;
    double step[MK];
    double bk1, tk, itk;
    double* out;   // MK merit values cFk_new
};

__global__ __launch_bounds__(BT) void k_merit_fin(const MeritFin a) {
    // All MK trial points in ONE pass over lam, zeta, wlk and ONE exchange: the per-thread sums, the
    // wave sums and the order in which the waves' sums are added are those of block_sum / scal_total
    // value by value (same bits); MK sequential passes with four block sums each took 16.5 us.
    __shared__ double redm[BT / 64][4 * MK];
    __shared__ double tot[4 * MK];
    const int M = a.P.m + a.P.n;
    const size_t mn = (size_t)a.P.m * a.P.n;
    const int L = M + (a.P.cls2 ? 1 : 0);
    double acc[4 * MK];
#pragma unroll
    for (int k = 0; k < 4 * MK; ++k) acc[k] = 0.0;
    for (int t = threadIdx.x; t < L; t += BT) {
        const double l0 = a.lam[t], zt = a.zeta[t], wlt = a.wlk[t];
        const bool tail = a.P.cls2 && t < M;
        const double wt = tail ? a.w[mn + t] : 0.0;
#pragma unroll
        for (int k = 0; k < MK; ++k) {
            const double lt = l0 + a.step[k] * zt;
            acc[k] += lt * lt;
            acc[MK + k] += wlt * lt;
            if (tail) {
                const double z = a.itk * (wt - lt);
                const double pz = z > 0.0 ? z : 0.0;
                acc[2 * MK + k] += pz * pz;
            }
        }
    }
    for (int b = threadIdx.x; b < a.pt.nblk; b += BT) {
#pragma unroll
        for (int k = 0; k < MK; ++k) acc[3 * MK + k] += a.pt.spart[(size_t)b * NSC + k];
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 4 * MK; ++k) {
        const double v = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) redm[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4 * MK) {
        double sgm = 0.0;
#pragma unroll
        for (int w = 0; w < BT / 64; ++w) sgm += redm[w][threadIdx.x];
        tot[threadIdx.x] = sgm;
    }
    __syncthreads();
    if (threadIdx.x < MK) {
        const int k = threadIdx.x;
        const double l2 = tot[k], wl = tot[MK + k], tp2 = tot[2 * MK + k];
        const double prox2 = tot[3 * MK + k] + tp2;
        a.out[k] = apd_merit_value(false, a.bk1, a.tk, l2, wl, prox2, 0.0, 0.0);   // :201-204
    }
}

ApdScal fetch_scal(ipd_apd* h) {
    ApdScal s;
    h->ctx->fetch_bytes(h->dscal, &s, sizeof(ApdScal));
    return s;
}

template <bool CLS2, bool GVEC, bool M3>
void launch_eval_t(ipd_apd* h, const Lam& lam, double itk) {
    OpEvalT<CLS2, GVEC, M3> op;
    op.P = h->P;
    op.w = h->w;
    op.s = h->s;
    op.lam = lam;
    op.itk = itk;
    launch_tiles(h, op);
}
void launch_eval(ipd_apd* h, bool merit3, const Lam& lam, double itk) {
    switch (apd_eval_kind(h->cls == 2, h->gama != nullptr, merit3)) {
        case EVAL_CLS2: return launch_eval_t<true, false, false>(h, lam, itk);
        case EVAL_GVEC_M3: return launch_eval_t<false, true, true>(h, lam, itk);
        case EVAL_GVEC: return launch_eval_t<false, true, false>(h, lam, itk);
        case EVAL_GS_M3: return launch_eval_t<false, false, true>(h, lam, itk);
        case EVAL_GS: return launch_eval_t<false, false, false>(h, lam, itk);
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
size_t apd_fpart_len(int L) { return (size_t)cdiv(L, EB) * NFS; }

void apd_begin(ipd_apd* h, int k) {
    ProfScope ps(h->ctx, PROF_BEGIN_END);
    const ApdStep st = apd_step(k, h->bk);
    h->ak = st.ak;
    h->bk1 = st.bk1;
    h->tk = st.tk;
    with_cost_source(h, [&](auto cs) {
        OpBeginT<decltype(cs)> op;
        op.P = h->P;
        op.u = h->u;
        op.v = h->v;
        op.w = h->w;
        op.ak = h->ak;
        op.bk = h->bk;
        op.ak2 = h->ak * h->ak;
        op.cs = cs;
        launch_tiles(h, op);
    });
    BeginFin f;
    f.pt = parts_of(h);
    f.P = h->P;
    f.u = h->u;
    f.v = h->v;
    f.w = h->w;
    f.lam = h->lam;
    f.b = h->b;
    f.wlk = h->wlk;
    f.ak = h->ak;
    f.bk = h->bk;
    f.ak2 = h->ak * h->ak;
    f.bk1 = h->bk1;
    f.ibk = 1.0 / h->bk;
    f.mu = h->mu;
    hipLaunchKernelGGL(k_begin_fin, dim3(1), dim3(BT), 0, h->ctx->stream, f);
    IPD_KERNEL_CHECK();
}

EvalRes apd_eval(ipd_apd* h, bool merit3, const double* lam_base, const double* zeta, double step, double* lam_out,
                 double* F_out, const double* F_old) {
    ProfScope ps(h->ctx, PROF_EVAL);
    const Lam lamv{lam_base, zeta, step};
    const double itk = 1.0 / h->tk;
    launch_eval(h, merit3, lamv, itk);
    EvalFin f;
    f.pt = parts_of(h);
    f.P = h->P;
    f.w = h->w;
    f.lam = lamv;
    f.wlk = h->wlk;
    f.Fold = F_old;
    f.lam_out = lam_out;
    f.F = F_out;
    f.tmask = h->tmask;
    f.bk1 = h->bk1;
    f.itk = itk;
    f.out = h->dscal;
    f.fpart = h->fpart;
    f.counter = h->counter;
    hipLaunchKernelGGL(k_eval_fin, dim3(cdiv(h->L, EB)), dim3(EB), 0, h->ctx->stream, f);
    IPD_KERNEL_CHECK();
    const ApdScal s = fetch_scal(h);
    EvalRes r;
    r.normF = std::sqrt(s.normF2);
    r.lam2 = s.lam2;
    r.wlk_lam = s.wlk_lam;
    r.prox2 = s.prox2;
    r.z2 = s.z2;
    r.zmp2 = s.zmp2;
    r.fold_zeta = s.fold_zeta;
    r.E = (long long)(s.count + 0.5);
    return r;
}

void apd_merit(ipd_apd* h, const double* lam_base, const double* zeta, const double step[MK], double merit[MK]) {
    ProfScope ps(h->ctx, PROF_EVAL);
    OpMerit op;
    op.P = h->P;
    op.w = h->w;
    op.lam = lam_base;
    op.zeta = zeta;
    op.itk = 1.0 / h->tk;
    MeritFin f;
    f.pt = parts_of(h);
    f.P = h->P;
    f.w = h->w;
    f.lam = lam_base;
    f.zeta = zeta;
    f.wlk = h->wlk;
    f.bk1 = h->bk1;
    f.tk = h->tk;
    f.itk = op.itk;
    f.out = h->merit;
    for (int k = 0; k < MK; ++k) op.step[k] = f.step[k] = step[k];
    launch_tiles(h, op);
    hipLaunchKernelGGL(k_merit_fin, dim3(1), dim3(BT), 0, h->ctx->stream, f);
    IPD_KERNEL_CHECK();
    h->ctx->fetch(h->merit, merit, MK);
}

void apd_end(ipd_apd* h, bool from_w, const double* src_u, const double* lam, double out_kkt[4], double* fx) {
    ProfScope ps(h->ctx, PROF_BEGIN_END);
    const Lam L{lam, nullptr, 0.0};
    with_cost_source(h, [&](auto cs) {
        if (from_w) {
            OpEndT<true, decltype(cs)> op;
            op.P = h->P;
            op.w = h->w;
            op.uold = h->u;
            op.unew = h->u2;
            op.v = h->v;
            op.lam = L;
            op.itk = 1.0 / h->tk;
            op.ak = h->ak;
            op.cs = cs;
            launch_tiles(h, op);
        } else {
            OpEndT<false, decltype(cs)> op;
            op.P = h->P;
            op.w = nullptr;
            op.uold = src_u;
            op.unew = nullptr;
            op.v = nullptr;
            op.lam = L;
            op.itk = 0.0;
            op.ak = 1.0;
            op.cs = cs;
            launch_tiles(h, op);
        }
    });
    EndFin f;
    f.pt = parts_of(h);
    f.P = h->P;
    f.from_w = from_w ? 1 : 0;
    f.w = h->w;
    f.uold = from_w ? h->u : src_u;
    f.unew = h->u2;
    f.v = h->v;
    f.lam = L;
    f.b = h->b;
    f.itk = from_w ? 1.0 / h->tk : 0.0;
    f.ak = from_w ? h->ak : 1.0;
    f.out = h->dscal;
    hipLaunchKernelGGL(k_end_fin, dim3(1), dim3(BT), 0, h->ctx->stream, f);
    IPD_KERNEL_CHECK();
    const ApdScal s = fetch_scal(h);
    out_kkt[0] = std::sqrt(s.kx2);
    out_kkt[1] = std::sqrt(s.kl2);
    out_kkt[2] = std::sqrt(s.ky2);
    out_kkt[3] = std::sqrt(s.kz2);
    *fx = s.fx;
}

float apd_bench_eval(ipd_apd* h, bool merit3, int reps) {
    ipd_ctx* ctx = h->ctx;
    const Lam lamv{h->lam, nullptr, 0.0};
    const double itk = 1.0 / h->tk;
    hipEvent_t e0, e1;
    IPD_HIP(hipEventCreate(&e0));
    IPD_HIP(hipEventCreate(&e1));
    launch_eval(h, merit3, lamv, itk);
    IPD_HIP(hipEventRecord(e0, ctx->stream));
    for (int r = 0; r < reps; ++r) launch_eval(h, merit3, lamv, itk);
    IPD_HIP(hipEventRecord(e1, ctx->stream));
    IPD_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    IPD_HIP(hipEventElapsedTime(&ms, e0, e1));
    IPD_HIP(hipEventDestroy(e0));
    IPD_HIP(hipEventDestroy(e1));
    return ms;
}
