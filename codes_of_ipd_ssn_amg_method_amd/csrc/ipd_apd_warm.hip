// A-ADMM warm start of the drivers on device-resident vectors:
// Class1/warmup_class1.m:22-96, Class2/warmup_class2.m:19-100.  Two passes of the tile walker
// (ipd_apd_tiles.h) per iteration, each with a one-workgroup epilogue; the per-iteration scalars are
// ipd_apd_script.h's (apd_warm_step).
#pragma clang fp contract(off)

#include "ipd_apd_state.h"
#include "ipd_kkt.h"

namespace {

// ---------------------------------------------------------------------------
// warm start: warmup_class1.m:57-77 / warmup_class2.m:57-85, two passes per iteration
// ---------------------------------------------------------------------------
// pass A: dd = etafk*wuk - ak^2*(wc + cAlk + sgk*cAw); partials of H*dd
template <class CS>   // CS: CostStored or CostFree<D> (ipd_apd_tiles.h)
struct OpWarmAT {
    static constexpr bool NEED_AX = true;
    static constexpr int FC = 4;
    Prob P;
    const double* x;
    const double* v;
    const double* wk;
    const double* pik;
    const double* l2;     // multiplier block of the splitting constraint u = w
    const double* hl1;    // hlk(1:L)
    const double* b;
    double* dd;
    WarmScal s;
    [[no_unique_address]] CS cs;
    struct Raw {
        double x, v, w, pi, l2, c, phi;
    };
    struct RowC {
        double pi, h2, b2;
        typename CS::Row x;
    };
    struct ColC {
        double bj, hj, q;
        typename CS::Col y;
    };
    __device__ void row_const(RowC& rc, int i) const {
        rc.pi = P.p[i];
        rc.h2 = hl1[P.n + i];
        rc.b2 = b[P.n + i];
        cs.row(rc.x, i);
    }
    __device__ void col_const(ColC& c, int j) const {
        c.bj = b[j];
        c.hj = hl1[j];
        c.q = P.q[j];
        cs.col(c.y, j);
    }
    __device__ void fetch(Raw& r, size_t idx) const {
        r.x = x[idx];
        r.v = v[idx];
        r.w = wk[idx];
        r.pi = pik[idx];
        r.l2 = l2[idx];
        r.c = CS::FREE ? 0.0 : P.c[idx];
        r.phi = P.cls2 ? P.phi[idx] : 0.0;
    }
    __device__ double compute(const Raw& r, const RowC& rc, const ColC& cc, size_t idx,
                              double* sc) const {
        const double wux = (s.ak * s.gk * r.v + s.gkmu * r.x) / s.etafk;              // :63
        const double hl2 = r.l2 - s.ibk * (r.x - r.w) + s.akbk * (-(r.pi - r.w));     // :65
        double atb = rc.pi * cc.bj + rc.b2 * cc.q;                                     // Atb
        double aty = rc.pi * cc.hj + rc.h2 * cc.q;
        const int M = P.m + P.n;
        double cAlk;
        if (P.cls2) {
            atb = atb + b[M] * r.phi;                                                  // Htb
            cAlk = hl2 + (aty + hl1[M] * r.phi);                                       // Class2 :66-67
        } else {
            cAlk = aty + hl2;                                                          // Class1 :66
        }
        const double cAw = -atb - r.w;
        const double d = s.etafk * wux - s.ak2 * (cs.value(r.c, rc.x, cc.y) + cAlk + s.sgk * cAw);          // :67
        dd[idx] = d;
        sc[3] += r.phi * d;
        return d;
    }
};

// pass B: xk1, vk1, wk1, pik1 and the splitting multiplier; partials of H*xk1.  H*vk1 follows in
// the epilogue from linearity, H*vk1 = H*xk1 + (H*xk1 - H*xk)/ak, without another pass.
struct OpWarmB {
    static constexpr bool NEED_AX = true;
    static constexpr int FC = 4;
    Prob P;
    const double* dd;
    const double* ff;     // invAAt / invHHt result (L entries)
    double* x;
    double* v;
    double* wk;
    double* pik;
    double* l2;
    WarmScal s;
    struct Raw {
        double d, x, w, pi, l2, phi, g;
    };
    struct RowC {
        double pi, f2;
    };
    struct ColC {
        double fj, q;
    };
    __device__ void row_const(RowC& rc, int i) const {
        rc.pi = P.p[i];
        rc.f2 = ff[P.n + i];
    }
    __device__ void col_const(ColC& c, int j) const {
        c.fj = ff[j];
        c.q = P.q[j];
    }
    __device__ void fetch(Raw& r, size_t idx) const {
        r.d = dd[idx];
        r.x = x[idx];
        r.w = wk[idx];
        r.pi = pik[idx];
        r.l2 = l2[idx];
        r.phi = P.cls2 ? P.phi[idx] : 0.0;
        r.g = P.gama ? P.gama[idx] : P.gs;
    }
    __device__ double compute(const Raw& r, const RowC& rc, const ColC& cc, size_t idx,
                              double* sc) const {
        double aty = rc.pi * cc.fj + rc.f2 * cc.q;
        if (P.cls2) aty = aty + ff[P.m + P.n] * r.phi;
        const double x1 = (r.d - aty) / s.tt_etafk;                                    // :70
        const double v1 = x1 + (x1 - r.x) / s.ak;                                      // :71
        const double wwk = (s.ak * r.pi + r.w) / s.iak1;                               // :62
        const double bl2 = r.l2 + s.akbk * (v1 - r.pi);                                // :72
        const double w1 = prox_of(P, wwk - s.prox_scale * (-bl2), r.g);                // :73
        const double pi1 = w1 + (w1 - r.w) / s.ak;                                     // :74
        const double l21 = r.l2 + s.akbk * (v1 - pi1);                                 // :75
        x[idx] = x1;
        v[idx] = v1;
        wk[idx] = w1;
        pik[idx] = pi1;
        l2[idx] = l21;
        sc[3] += r.phi * x1;
        return x1;
    }
};

// epilogue 1 of the warm start: Hdd = [Ax(dd_x)+dd_tail ; phi'dd_x], tails of dd
struct WarmFinA {
    Parts pt;
    Prob P;
    const double* x;
    const double* v;
    const double* wk;
    const double* pik;
    const double* l2;
    const double* hl1;
    const double* b;
    double* dd;
    double* Hdd;
    WarmScal s;
};

__global__ __launch_bounds__(BT) void k_warm_fin_a(const WarmFinA a) {
    __shared__ double red[16];
    const int M = a.P.m + a.P.n;
    const size_t mn = (size_t)a.P.m * a.P.n;
    const double phid = a.P.cls2 ? scal_total(a.pt, 3, red) : 0.0;
    const WarmScal& s = a.s;
    for (int t = threadIdx.x; t < M; t += BT) {
        double h = ax_entry(a.pt, t);
        if (a.P.cls2) {
            const size_t id = mn + t;
            const double wux = (s.ak * s.gk * a.v[id] + s.gkmu * a.x[id]) / s.etafk;
            const double hl2 = a.l2[id] - s.ibk * (a.x[id] - a.wk[id]) +
                               s.akbk * (-(a.pik[id] - a.wk[id]));
            const double cAlk = hl2 + a.hl1[t];          // [Aty(..)+..*phi ; hlk(1:n+m)] tail
            const double cAw = -a.b[t] - a.wk[id];       // Htb tail = b(1:n+m)
            const double d = s.etafk * wux - s.ak2 * (0.0 + cAlk + s.sgk * cAw);
            a.dd[id] = d;
            h = h + d;                                   // Ax(dd_x) + dd(mn+1:end)
        }
        a.Hdd[t] = h;
    }
    if (a.P.cls2 && threadIdx.x == 0) a.Hdd[M] = phid;
}

// hlk(1:L) = lk1 - 1/bk*(H*uk - b)        (the z0 block of :65 adds nothing)
__global__ __launch_bounds__(BT) void k_warm_hl1(int L, const double* __restrict__ lk1,
                                                 const double* __restrict__ Hu,
                                                 const double* __restrict__ b, double ibk,
                                                 double akbk, double* __restrict__ hl1) {
    for (int t = threadIdx.x; t < L; t += BT)
        hl1[t] = lk1[t] - ibk * (Hu[t] - b[t]) + akbk * 0.0;
}

// epilogue 2: tails of pass B, H*xk1, H*vk1 and lk1(1:L) += ak/bk*(H*vk1 - b)
struct WarmFinB {
    Parts px;   // partials of xk1
    Prob P;
    const double* dd;
    const double* ff;
    double* x;
    double* v;
    double* wk;
    double* pik;
    double* l2;
    const double* b;
    double* lk1;
    double* Hx;
    WarmScal s;
};

__global__ __launch_bounds__(BT) void k_warm_fin_b(const WarmFinB a) {
    __shared__ double red[16];
    const int M = a.P.m + a.P.n;
    const size_t mn = (size_t)a.P.m * a.P.n;
    const double phix = a.P.cls2 ? scal_total(a.px, 3, red) : 0.0;
    const WarmScal& s = a.s;
    for (int t = threadIdx.x; t < M; t += BT) {
        double hx = ax_entry(a.px, t);
        if (a.P.cls2) {
            const size_t id = mn + t;
            const double x0 = a.x[id], w0 = a.wk[id], pi0 = a.pik[id], l20 = a.l2[id];
            const double x1 = (a.dd[id] - a.ff[t]) / s.tt_etafk;           // [..; ff(1:m+n)] tail
            const double v1 = x1 + (x1 - x0) / s.ak;
            const double wwk = (s.ak * pi0 + w0) / s.iak1;
            const double bl2 = l20 + s.akbk * (v1 - pi0);
            const double arg = wwk - s.prox_scale * (-bl2);
            const double w1 = arg > 0.0 ? arg : 0.0;
            const double pi1 = w1 + (w1 - w0) / s.ak;
            a.x[id] = x1;
            a.v[id] = v1;
            a.wk[id] = w1;
            a.pik[id] = pi1;
            a.l2[id] = l20 + s.akbk * (v1 - pi1);
            hx = hx + x1;
        }
        const double hv = hx + (hx - a.Hx[t]) / s.ak;
        a.Hx[t] = hx;
        a.lk1[t] = a.lk1[t] + s.akbk * (hv - a.b[t]);                      // :75
    }
    if (a.P.cls2 && threadIdx.x == 0) {
        const double phiv = phix + (phix - a.Hx[M]) / s.ak;
        a.Hx[M] = phix;
        a.lk1[M] = a.lk1[M] + s.akbk * (phiv - a.b[M]);
    }
}

}  // namespace

void apd_warmup(ipd_apd* h, double res, long long maxit) {
    (void)res;  // the reference's residual test is commented out (:82-93): only maxit acts
    ipd_ctx* ctx = h->ctx;
    CallScope scope(ctx);
    Arena& tmp = *ctx->scratch;
    const size_t U = h->U;
    const int L = h->L;
    double* x = h->u;
    double* v = h->v;
    double* dd = h->w;
    double* wk = tmp.alloc<double>(U);
    double* pik = tmp.alloc<double>(U);
    double* l2 = tmp.alloc<double>(U);
    double* lk1 = tmp.alloc<double>((size_t)L);
    double* hl1 = tmp.alloc<double>((size_t)L);
    double* Hx = tmp.alloc<double>((size_t)L);
    double* Hdd = tmp.alloc<double>((size_t)L);
    double* ff = tmp.alloc<double>((size_t)L);
    for (double* a : {x, v, wk, pik, l2}) IPD_HIP(hipMemsetAsync(a, 0, U * sizeof(double), ctx->stream));
    for (double* a : {lk1, Hx}) IPD_HIP(hipMemsetAsync(a, 0, (size_t)L * sizeof(double), ctx->stream));
    const double muf = 0.0;
    double gk = 1.0, bk = 1.0;
    for (long long it = 1; it <= maxit; ++it) {
        const WarmStep ws = apd_warm_step(gk, bk, muf);
        const WarmScal& s = ws.s;
        hipLaunchKernelGGL(k_warm_hl1, dim3(1), dim3(BT), 0, ctx->stream, L, (const double*)lk1,
                           (const double*)Hx, (const double*)h->b, s.ibk, s.akbk, hl1);
        IPD_KERNEL_CHECK();
        with_cost_source(h, [&](auto cs) {
            OpWarmAT<decltype(cs)> a;
            a.P = h->P;
            a.x = x;
            a.v = v;
            a.wk = wk;
            a.pik = pik;
            a.l2 = l2;
            a.hl1 = hl1;
            a.b = h->b;
            a.dd = dd;
            a.s = s;
            a.cs = cs;
            launch_tiles(h, a);
        });
        WarmFinA fa;
        fa.pt = parts_of(h);
        fa.P = h->P;
        fa.x = x;
        fa.v = v;
        fa.wk = wk;
        fa.pik = pik;
        fa.l2 = l2;
        fa.hl1 = hl1;
        fa.b = h->b;
        fa.dd = dd;
        fa.Hdd = Hdd;
        fa.s = s;
        hipLaunchKernelGGL(k_warm_fin_a, dim3(1), dim3(BT), 0, ctx->stream, fa);
        IPD_KERNEL_CHECK();
        {
            CallScope inner(ctx);
            if (h->cls == 2)
                kkt_inv_hht_pre(ctx, Hdd, h->p, h->q, h->m, h->n, ws.sg, h->phi_l, h->phi_part,
                                h->phi_npart, ff);                                // Class2 :72
            else
                kkt_inv_aat(ctx, Hdd, h->p, h->q, h->m, h->n, ws.sg, ws.sg, ff);  // Class1 :70
            OpWarmB b;
            b.P = h->P;
            b.dd = dd;
            b.ff = ff;
            b.x = x;
            b.v = v;
            b.wk = wk;
            b.pik = pik;
            b.l2 = l2;
            b.s = s;
            launch_tiles(h, b);
            WarmFinB fb;
            fb.px = parts_of(h);
            fb.P = h->P;
            fb.dd = dd;
            fb.ff = ff;
            fb.x = x;
            fb.v = v;
            fb.wk = wk;
            fb.pik = pik;
            fb.l2 = l2;
            fb.b = h->b;
            fb.lk1 = lk1;
            fb.Hx = Hx;
            fb.s = s;
            hipLaunchKernelGGL(k_warm_fin_b, dim3(1), dim3(BT), 0, ctx->stream, fb);
            IPD_KERNEL_CHECK();
        }
        gk = ws.gk1;
        bk = ws.bk1;
    }
    // driver state: xk = xk0, vk = xk, lk = lk0, bk = 1      (Class1 :59-60,35)
    copy_dev(h, h->v, h->u, U);
    copy_dev(h, h->lam, lk1, (size_t)L);
    ctx->sync();
    h->bk = 1.0;
    h->k = 0;
    h->have_kkt = false;
    h->converged = false;
}
