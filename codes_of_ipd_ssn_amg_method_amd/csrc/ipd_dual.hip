// The dual certificate where the multiplier lives (ipd_apd_dual, ipd_apd_dual_dev): the
// c-transform of one side of lam = [alpha (n); beta (m)(; tau)] with its arg-max map, and the dual value, the smallest
// reduced cost and the duality gap of the result.  Nothing mn-sized crosses the host boundary and nothing of the
// workspace is written: partials and results live in the context's scratch arena.
//
//   transform  one streaming read of c (and phi) on the column-group walk of DESIGN.md section 4j (ipd_walk_geo.h,
//              ipd_walk_dev.h).  A candidate is
//                side 0   t(i,j) = ((-c(i,j) [- tau*phi(i,j)]) - p_i*alpha_j) / q_j     beta^_i  = max_j t(i,j)
//                side 1   t(i,j) = ((-c(i,j) [- tau*phi(i,j)]) - q_j*beta_i)  / p_i     alpha^_j = max_i t(i,j)
//              every operation one IEEE operation in the order written; a NaN counts as -inf; the key of the
//              maximum is (value descending, index ascending), which is associative: any tree gives the same bits.
//     side 0   the running (max, arg max) stays in registers over the column group and leaves as one partial per
//              (group, row).
//     side 1   a lane holds p_i and beta_i; per chunk one colmax16 butterfly -- colsum16 of the tile walker on the
//              (value, index) key -- gives the wave's 16 column maxima, one partial per (segment slot, column).
//   finish     one thread per entry of lam_out: the new side combines its partials in index order (class 2: clamped
//              at 0), the held side is copied (class 2: clamped at 0), tau passes through.
//   evaluate   one pass forms d(i,j) = ((c + p_i*alpha_j) + q_j*beta_i) [+ tau*phi] and keeps, per workgroup, the
//              smallest d with its first column-major place, the count of d < 0, sum gama*(-d) over d < 0 (finite
//              gama only) and, with primal = 1, sum c*x -- the only case that reads u.
//   last       one workgroup: the evaluation's partials in a fixed shape, class 2's alpha and beta blocks of d,
//              -<b, lam> (thread t adds entries t, t + 256, ... in order, then a fixed tree), the dual value and gap.
//
// The host side is cut into the stages of ipd_apd_state.h (apd_dual_finish, apd_dual_eval, apd_dual_last):
// ipd_bracket.hip walks c itself, for both sides at once, and has them launch what this unit defines.  The keys and
// colmax16: ipd_dual_dev.h.
//
// Geometry and every index: ipd_dual_geo.h.  Deterministic: maxima and minima are order-independent, every sum has a
// fixed shape, no float atomics -- two calls give the same bits, and so do the host and the device entry.
#pragma clang fp contract(off)

#include <cmath>
#include <limits>
#include <vector>

#include "ipd_apd_state.h"
#include "ipd_dual_dev.h"

namespace {

// ---------------------------------------------------------------------------
// transform
// ---------------------------------------------------------------------------
// the cost source CS of a walking kernel (CostStored or CostFree<D>, ipd_apd_tiles.h) is an argument of its own
struct DuWalk {
    DuGeo g;
    int cls2;
    const double* c;     // CostStored
    const double* phi;   // class 2
    const double* p;
    const double* q;
    const double* lam;   // alpha at lam, beta at lam + n, class 2: tau at lam[n + m]
    double* pv;          // du_part_index
    int* pi;
};

// side 0: hold alpha, produce beta^
template <class CS>
__global__ __launch_bounds__(256) void k_du_rows(const DuWalk a, const CS cs) {
    const DuGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const double pi = a.p[t.ic];
    const double tau = a.cls2 ? a.lam[g.n + g.m] : 0.0;
    typename CS::Row crow;
    cs.row(crow, t.ic);
    double bv = -INFINITY;
    int bj = walk_chunk_col(t.grp, 0);   // below n; stays when every candidate of the group is -inf
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        double cr[TC], fr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const size_t idx = walk_place(t, g, j0, jj);
            cr[jj] = CS::FREE ? 0.0 : a.c[idx];
            fr[jj] = a.cls2 ? a.phi[idx] : 0.0;
        }
        const int jl = walk_lane_col(t, g, j0);   // alpha, q (and the coordinates)
        double al = a.lam[jl];
        if (a.cls2) al = walk_pos(al);
        const double ql = a.q[jl];
        typename CS::Col clane;
        cs.col(clane, jl);
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const double aj = __shfl(al, jj), qj = __shfl(ql, jj);
            typename CS::Col ccol;
            cs.col_of_lane(ccol, clane, jj);
            double v = -cs.value(cr[jj], crow, ccol);
            if (a.cls2) {
                const double tf = tau * fr[jj];
                v = v - tf;
            }
            const double pa = pi * aj;
            v = v - pa;
            v = v / qj;
            const double cand = (j0 + jj < g.n && v == v) ? v : -INFINITY;   // a NaN never wins
            if (cand > bv) {   // columns ascend: the first of equal maxima stays
                bv = cand;
                bj = j0 + jj;
            }
        }
    }
    if (t.in_i) {
        a.pv[du_part_index(g, t.grp, t.i)] = bv;
        a.pi[du_part_index(g, t.grp, t.i)] = bj;
    }
}

// side 1: hold beta, produce alpha^
template <class CS>
__global__ __launch_bounds__(256) void k_du_cols(const DuWalk a, const CS cs) {
    const DuGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const int slot = t.slot();   // of a segment without rows too: its maxima are (-inf, DU_NOIDX)
    const double pi = a.p[t.ic];
    double bi = a.lam[g.n + t.ic];
    if (a.cls2) bi = walk_pos(bi);
    const double tau = a.cls2 ? a.lam[g.n + g.m] : 0.0;
    typename CS::Row crow;
    cs.row(crow, t.ic);
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        double cr[TC], fr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const size_t idx = walk_place(t, g, j0, jj);
            cr[jj] = CS::FREE ? 0.0 : a.c[idx];
            fr[jj] = a.cls2 ? a.phi[idx] : 0.0;
        }
        const int jl = walk_lane_col(t, g, j0);
        const double ql = a.q[jl];
        typename CS::Col clane;
        cs.col(clane, jl);
        double xv[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const double qj = __shfl(ql, jj);
            typename CS::Col ccol;
            cs.col_of_lane(ccol, clane, jj);
            double v = -cs.value(cr[jj], crow, ccol);
            if (a.cls2) {
                const double tf = tau * fr[jj];
                v = v - tf;
            }
            const double qb = qj * bi;
            v = v - qb;
            v = v / pi;
            xv[jj] = (t.in_i && j0 + jj < g.n && v == v) ? v : -INFINITY;
        }
        double mv;
        int mi, col;
        colmax16(xv, t.in_i ? t.i : DU_NOIDX, t.lane, mv, mi);
        if (walk_col_owner(t, g, j0, col)) {
            a.pv[du_part_index(g, slot, col)] = mv;
            a.pi[du_part_index(g, slot, col)] = mi;
        }
    }
}

struct DuFin {
    DuGeo g;
    int cls2;
    const double* pv;
    const int* pi;
    const double* lam;
    double* lam_out;   // L entries
    int* arg;          // R entries or nullptr
};

constexpr int DU_FB = 16;   // partials a finishing thread has in flight

template <bool ARG>
__global__ __launch_bounds__(256) void k_du_fin(const DuFin a) {
    const DuGeo& g = a.g;
    const int M = g.n + g.m;
    const int t = blockIdx.x * 256 + threadIdx.x;   // position in lam = [alpha (n); beta (m)(; tau)]
    if (t >= M + a.cls2) return;
    const bool made = g.own.side == 0 ? (t >= g.n && t < M) : t < g.n;
    if (!made) {
        double v = a.lam[t];
        if (a.cls2 && t < M) v = walk_pos(v);   // the held side; tau passes through
        a.lam_out[t] = v;
        return;
    }
    const int r = g.own.side == 0 ? t - g.n : t;
    const int S = du_part_count(g);
    double bv = a.pv[du_part_index(g, 0, r)];
    int bi = a.pi[du_part_index(g, 0, r)];
    int s = 1;
    for (; s + DU_FB <= S; s += DU_FB) {   // loads go out DU_FB at a time, as sum_strided's: a plain loop pays a round trip each
        double v[DU_FB];
        int ix[DU_FB];
#pragma unroll
        for (int k = 0; k < DU_FB; ++k) {
            v[k] = a.pv[du_part_index(g, s + k, r)];
            ix[k] = a.pi[du_part_index(g, s + k, r)];
        }
#pragma unroll
        for (int k = 0; k < DU_FB; ++k) du_merge(bv, bi, v[k], ix[k]);
    }
    for (; s < S; ++s) du_merge(bv, bi, a.pv[du_part_index(g, s, r)], a.pi[du_part_index(g, s, r)]);
    if (a.cls2) bv = walk_pos(bv);
    a.lam_out[t] = bv;
    if (ARG) a.arg[r] = bi;
}

// ---------------------------------------------------------------------------
// evaluate
// ---------------------------------------------------------------------------
struct DuEval {
    DuGeo g;
    int cls2;
    int cap_on;           // class 1 with finite gama: sum gama*(-d) over d < 0
    const double* c;      // CostStored
    const double* phi;    // class 2
    const double* gama;   // class 1, nullptr -> gs
    double gs;
    const double* p;
    const double* q;
    const double* lam;
    const double* x;      // PRIMAL
    DuEvalPart* part;     // walk_block_index
};

template <bool PRIMAL, class CS>
__global__ __launch_bounds__(256) void k_du_eval(const DuEval a, const CS cs) {
    __shared__ DuEvalPart red[APD_WAVES];
    const DuGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const double pi = a.p[t.ic];
    const double bi = a.lam[g.n + t.ic];
    const double tau = a.cls2 ? a.lam[g.n + g.m] : 0.0;
    const bool gvec = a.cap_on && a.gama;
    typename CS::Row crow;
    cs.row(crow, t.ic);
    double dmin = INFINITY, cap = 0.0, fv = 0.0;
    long long didx = DU_NOPLACE;
    int nneg = 0;
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        double cr[TC], fr[TC], gr[TC], xr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const size_t idx = walk_place(t, g, j0, jj);
            cr[jj] = CS::FREE ? 0.0 : a.c[idx];
            xr[jj] = PRIMAL ? a.x[idx] : 0.0;
            fr[jj] = a.cls2 ? a.phi[idx] : 0.0;
            gr[jj] = gvec ? a.gama[idx] : a.gs;
        }
        const int jl = walk_lane_col(t, g, j0);
        const double al = a.lam[jl];
        const double ql = a.q[jl];
        typename CS::Col clane;
        cs.col(clane, jl);
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const double aj = __shfl(al, jj), qj = __shfl(ql, jj);
            typename CS::Col ccol;
            cs.col_of_lane(ccol, clane, jj);
            const double cv = cs.value(cr[jj], crow, ccol);
            const double pa = pi * aj;
            double d = cv + pa;
            const double qb = qj * bi;
            d = d + qb;
            if (a.cls2) {
                const double tf = tau * fr[jj];
                d = d + tf;
            }
            const bool valid = t.in_i && j0 + jj < g.n;
            if (valid && d < dmin) {   // columns ascend: the first of equal minima stays; a NaN never wins
                dmin = d;
                didx = (long long)(j0 + jj) * g.m + t.i;
            }
            const bool neg = valid && d < 0.0;
            nneg += neg ? 1 : 0;
            if (a.cap_on) {
                const double w = gr[jj] * (-d);
                cap += neg ? w : 0.0;
            }
            if (PRIMAL) {
                const double cx = cv * xr[jj];
                fv += valid ? cx : 0.0;
            }
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        du_merge_min(dmin, didx, __shfl_xor(dmin, s), __shfl_xor(didx, s));
        nneg += __shfl_xor(nneg, s);
    }
    cap = wave_sum(cap);
    fv = wave_sum(fv);
    if (t.lane == 0) {
        red[t.wv].dmin = dmin;
        red[t.wv].idx = didx;
        red[t.wv].nneg = nneg;
        red[t.wv].cap = cap;
        red[t.wv].fval = fv;
    }
    __syncthreads();
    if (t.tid == 0) {
        DuEvalPart r = red[0];
#pragma unroll
        for (int w = 1; w < APD_WAVES; ++w) {
            du_merge_min(r.dmin, r.idx, red[w].dmin, red[w].idx);
            r.nneg += red[w].nneg;
            r.cap += red[w].cap;
            r.fval += red[w].fval;
        }
        a.part[walk_block_index(g, t.ib, t.grp)] = r;
    }
}

struct DuLast {
    DuGeo g;
    int cls2, primal;
    const DuEvalPart* part;
    const double* b;     // [r; l(; mu)]
    const double* lam;   // the multiplier that was evaluated
    ipd_dual_stats* out;
};

__global__ __launch_bounds__(256) void k_du_last(const DuLast a) {
    __shared__ DuEvalPart red[APD_WAVES];
    __shared__ double redb[APD_WAVES];
    const DuGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int M = g.n + g.m, L = M + a.cls2, nblk = walk_blocks(g);
    const long long mn = (long long)g.m * g.n;
    DuEvalPart r;
    r.dmin = INFINITY;
    r.idx = DU_NOPLACE;
    r.nneg = 0;
    r.cap = r.fval = 0.0;
    for (int k = tid; k < nblk; k += 256) {
        const DuEvalPart o = a.part[k];
        du_merge_min(r.dmin, r.idx, o.dmin, o.idx);
        r.nneg += o.nneg;
        r.cap += o.cap;
        r.fval += o.fval;
    }
    if (a.cls2)   // the blocks d_y = alpha, d_z = beta follow the x block
        for (int k = tid; k < M; k += 256) {
            const double v = a.lam[k];
            du_merge_min(r.dmin, r.idx, v, mn + k);
            r.nneg += v < 0.0 ? 1 : 0;
        }
    double bs = 0.0;
    int k0 = tid;
    for (; k0 + (DU_FB - 1) * 256 < L; k0 += DU_FB * 256) {   // the same order of additions, the loads in one burst
        double t[DU_FB];
#pragma unroll
        for (int k = 0; k < DU_FB; ++k) t[k] = a.b[k0 + k * 256] * a.lam[k0 + k * 256];
#pragma unroll
        for (int k = 0; k < DU_FB; ++k) bs += t[k];
    }
    for (; k0 < L; k0 += 256) {
        const double t = a.b[k0] * a.lam[k0];
        bs += t;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        du_merge_min(r.dmin, r.idx, __shfl_xor(r.dmin, s), __shfl_xor(r.idx, s));
        r.nneg += __shfl_xor(r.nneg, s);
    }
    r.cap = wave_sum(r.cap);
    r.fval = wave_sum(r.fval);
    bs = wave_sum(bs);
    if (lane == 0) {
        red[wv] = r;
        redb[wv] = bs;
    }
    __syncthreads();
    if (tid == 0) {
        r = red[0];
        bs = redb[0];
#pragma unroll
        for (int w = 1; w < APD_WAVES; ++w) {
            du_merge_min(r.dmin, r.idx, red[w].dmin, red[w].idx);
            r.nneg += red[w].nneg;
            r.cap += red[w].cap;
            r.fval += red[w].fval;
            bs += redb[w];
        }
        ipd_dual_stats st;
        st.bterm = -bs;
        st.cap = r.cap;
        st.dual = st.bterm - st.cap;
        st.dmin = r.dmin;
        const bool in_x = r.idx < mn;
        st.imin = in_x ? r.idx % g.m : -1;
        st.jmin = in_x ? r.idx / g.m : -1;
        st.nneg = r.nneg;
        const double nan = std::numeric_limits<double>::quiet_NaN();
        st.fval = a.primal ? r.fval : nan;
        st.gap = a.primal ? st.fval - st.dual : nan;
        *a.out = st;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
}  // namespace

bool apd_dual_cap_on(const ipd_apd* h) { return h->cls == 1 && (h->gama || std::isfinite(h->P.gs)); }

// the divider of a transform, q (side 0) or p (side 1), must be positive and finite: read once per workspace (p and q
// never change after the create) and remembered
void apd_dual_check_divider(ipd_apd* h, int side) {
    int8_t& known = h->dual_divider[side];
    if (!known) {
        const size_t cnt = side ? (size_t)h->m : (size_t)h->n;
        std::vector<double> v(cnt);
        h->ctx->fetch(side ? h->p : h->q, v.data(), cnt);
        known = 1;
        for (double x : v)
            if (!(x > 0.0) || !std::isfinite(x)) known = -1;
    }
    IPD_REQUIRE(known > 0, IPD_E_ARG,
                side ? "ipd_apd_dual: side 1 divides by p, which has an entry that is <= 0 or not finite"
                     : "ipd_apd_dual: side 0 divides by q, which has an entry that is <= 0 or not finite");
}

void apd_dual_finish(ipd_apd* h, int side, const double* pv, const int* pi, const double* lam_dev, double* lam_out_dev,
                     int32_t* arg_dev) {
    DuFin f;
    f.g = du_make_geo(h->m, h->n, side);
    f.cls2 = h->cls == 2 ? 1 : 0;
    f.pv = pv;
    f.pi = pi;
    f.lam = lam_dev;
    f.lam_out = lam_out_dev;
    f.arg = arg_dev;
    const dim3 fgrid(cdiv(h->L, 256));
    if (arg_dev)
        hipLaunchKernelGGL(k_du_fin<true>, fgrid, dim3(256), 0, h->ctx->stream, f);
    else
        hipLaunchKernelGGL(k_du_fin<false>, fgrid, dim3(256), 0, h->ctx->stream, f);
    IPD_KERNEL_CHECK();
}

void apd_dual_last(ipd_apd* h, const DuEvalPart* part, const double* lam_eval, int primal, ipd_dual_stats* out_dev) {
    DuLast l;
    l.g = du_make_geo(h->m, h->n, 0);   // the shape and the grid: the side is not read
    l.cls2 = h->cls == 2 ? 1 : 0;
    l.primal = primal;
    l.part = part;
    l.b = h->b;
    l.lam = lam_eval;
    l.out = out_dev;
    hipLaunchKernelGGL(k_du_last, dim3(1), dim3(256), 0, h->ctx->stream, l);
    IPD_KERNEL_CHECK();
}

void apd_dual_eval(ipd_apd* h, const double* lam_eval, int primal, DuEvalPart* part) {
    const DuGeo g = du_make_geo(h->m, h->n, 0);
    DuEval e;
    e.g = g;
    e.cls2 = h->cls == 2 ? 1 : 0;
    e.cap_on = apd_dual_cap_on(h) ? 1 : 0;
    e.c = h->c;
    e.phi = h->phi;
    e.gama = h->gama;
    e.gs = h->P.gs;
    e.p = h->p;
    e.q = h->q;
    e.lam = lam_eval;
    e.x = h->u;   // class 2: the x block of uk comes first
    e.part = part;
    const dim3 grid(g.nib, g.ng);
    with_cost_source(h, [&](auto cs) {
        if (primal)
            hipLaunchKernelGGL((k_du_eval<true, decltype(cs)>), grid, dim3(256), 0, h->ctx->stream, e, cs);
        else
            hipLaunchKernelGGL((k_du_eval<false, decltype(cs)>), grid, dim3(256), 0, h->ctx->stream, e, cs);
    });
    IPD_KERNEL_CHECK();
}

namespace {

void check_args(ipd_apd* h, int32_t side, int32_t primal, const ipd_dual_stats* st) {
    IPD_REQUIRE(h && st, IPD_E_ARG, "ipd_apd_dual: NULL argument");
    IPD_REQUIRE(side >= -1 && side <= 1, IPD_E_ARG, "ipd_apd_dual: side must be -1, 0 or 1");
    IPD_REQUIRE(primal == 0 || primal == 1, IPD_E_ARG, "ipd_apd_dual: primal must be 0 or 1");
    IPD_REQUIRE(side < 0 || !apd_dual_cap_on(h), IPD_E_UNSUPPORTED,
                "ipd_apd_dual: with finite gama every multiplier is feasible; only side = -1 applies");
}

// all launches of a call on the context's stream; *st is read back (the stream is waited for).  lam_dev: L entries;
// lam_out_dev: L entries or nullptr; arg_dev: du_out_rows entries or nullptr (both ignored for side < 0)
void dual_dev(ipd_apd* h, const double* lam_dev, int side, int primal, double* lam_out_dev, int32_t* arg_dev,
              ipd_dual_stats* st) {
    ipd_ctx* ctx = h->ctx;
    Arena& S = *ctx->scratch;
    const DuGeo g = du_make_geo(h->m, h->n, side > 0 ? 1 : 0);
    const dim3 grid(g.nib, g.ng);
    const int cls2 = h->cls == 2 ? 1 : 0;
    const double* lam_eval = lam_dev;
    if (side >= 0) {
        double* pv = S.alloc<double>(du_part_len(g));
        int* pi = S.alloc<int>(du_part_len(g));
        if (!lam_out_dev) lam_out_dev = S.alloc<double>((size_t)h->L);
        DuWalk a;
        a.g = g;
        a.cls2 = cls2;
        a.c = h->c;
        a.phi = h->phi;
        a.p = h->p;
        a.q = h->q;
        a.lam = lam_dev;
        a.pv = pv;
        a.pi = pi;
        with_cost_source(h, [&](auto cs) {
            if (side == 0)
                hipLaunchKernelGGL((k_du_rows<decltype(cs)>), grid, dim3(256), 0, ctx->stream, a, cs);
            else
                hipLaunchKernelGGL((k_du_cols<decltype(cs)>), grid, dim3(256), 0, ctx->stream, a, cs);
        });
        IPD_KERNEL_CHECK();
        apd_dual_finish(h, side, pv, pi, lam_dev, lam_out_dev, arg_dev);
        lam_eval = lam_out_dev;
    }
    DuEvalPart* part = reinterpret_cast<DuEvalPart*>(
        S.alloc<double>((size_t)walk_blocks(g) * (sizeof(DuEvalPart) / sizeof(double))));
    apd_dual_eval(h, lam_eval, primal, part);
    ipd_dual_stats* out = reinterpret_cast<ipd_dual_stats*>(S.alloc<double>(APD_STATS_DOUBLES));
    apd_dual_last(h, part, lam_eval, primal, out);
    ctx->fetch_bytes(out, st, sizeof(ipd_dual_stats));
}
static_assert(sizeof(ipd_dual_stats) <= APD_STATS_DOUBLES * sizeof(double) && sizeof(DuEvalPart) % sizeof(double) == 0,
              "dual_dev sizes the result and the partials in doubles");

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_dual_dev(ipd_apd* h, const double* lam_dev, int32_t side, int32_t primal, double* lam_out_dev,
                                int32_t* arg_dev, ipd_dual_stats* st) {
    return ipd_guard([&] {
        check_args(h, side, primal, st);
        CallScope scope(h->ctx);
        if (side >= 0) apd_dual_check_divider(h, side);
        ipd_dual_stats got;
        dual_dev(h, lam_dev ? lam_dev : h->lam, side, primal, lam_out_dev, arg_dev, &got);
        h->ctx->sync();   // the scratch arrays are the next call's
        *st = got;
    });
}

extern "C" int ipd_apd_dual(ipd_apd* h, const double* lam, int32_t side, int32_t primal, double* lam_out,
                            int32_t* arg, ipd_dual_stats* st) {
    return ipd_guard([&] {
        check_args(h, side, primal, st);
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        if (side >= 0) apd_dual_check_divider(h, side);
        Arena& S = *ctx->scratch;
        const size_t L = (size_t)h->L, R = side > 0 ? (size_t)h->n : (size_t)h->m;
        const double* lam_dev = h->lam;
        if (lam) {
            double* up = S.alloc<double>(L);
            ctx->upload(up, lam, L);
            lam_dev = up;
        }
        double* out_dev = side >= 0 && lam_out ? S.alloc<double>(L) : nullptr;
        int32_t* arg_dev = side >= 0 && arg ? S.alloc<int32_t>(R) : nullptr;
        ipd_dual_stats got;
        dual_dev(h, lam_dev, side, primal, out_dev, arg_dev, &got);
        if (out_dev) ctx->fetch(out_dev, lam_out, L);
        if (arg_dev) ctx->fetch(arg_dev, arg, R);
        ctx->sync();
        *st = got;
    });
}
