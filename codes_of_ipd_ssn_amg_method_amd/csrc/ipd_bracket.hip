// Both certificates of a state in one call (ipd_apd_bracket, ipd_apd_bracket_dev): the dual
// certificate of ipd_dual.hip for both sides and the primal certificate of ipd_round.hip for both sides, reading
// once what the two sides share, with one read-back.  The drivers' probe of the certified gap (ipd_driver.hip) is
// this call.
//
//   transform  k_du_both: one walk over c (class 2: and phi) forms -c [- tau*phi] once per entry and from it the
//              candidates of both sides with the operations of k_du_rows and k_du_cols; the row candidates stay in
//              registers as there, the column candidates go through colmax16, and both partial sets are written.
//              k_du_fin (ipd_dual.hip) then runs once per side.
//   evaluate   k_du_eval2: one read of c and x evaluates the two repaired multipliers -- two (dmin, place, nneg),
//              which do not depend on an order under their key, and one sum c*x, accumulated as k_du_eval<true>
//              does.  k_du_last (ipd_dual.hip) then runs once per side.
//   rounding   pass A once, k_rd_fin<0> for side 0 and side 1 straight after it, then the rest of each side with
//              ipd_round.hip's kernels.
//   result     the two ipd_dual_stats and the two ipd_round_stats lie together and come back in one fetch; the host
//              picks (ipd_apd_script.h), and the writing kernels are enqueued for the winner only.
// Per-entry operations and summation orders are the single calls': the bits are theirs.
#pragma clang fp contract(off)

#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>

#include "ipd_apd_state.h"
#include "ipd_dual_dev.h"

namespace {

struct DuBoth {
    DuGeo g;             // the side is not read: the row partials have side 0's layout, the column partials side 1's
    int cls2;
    const double* c;     // CostStored
    const double* phi;   // class 2
    const double* p;
    const double* q;
    const double* lam;   // alpha at lam, beta at lam + n, class 2: tau at lam[n + m]
    double* pv;          // side 0's partials (a new beta, walk_row_part_len entries), then side 1's (a new alpha)
    int* pi;
};

template <class CS>
__global__ __launch_bounds__(256) void k_du_both(const DuBoth a, const CS cs) {
    const DuGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const int slot = t.slot();   // of a segment without rows too: its maxima are (-inf, DU_NOIDX)
    const double pi = a.p[t.ic];
    double bi = a.lam[g.n + t.ic];
    if (a.cls2) bi = walk_pos(bi);
    const double tau = a.cls2 ? a.lam[g.n + g.m] : 0.0;
    typename CS::Row crow;
    cs.row(crow, t.ic);
    double bv = -INFINITY;
    // the arg max as (first column of its chunk, column within the chunk): below n, and the group's first column
    // when every candidate of the group is -inf
    int bj0 = walk_chunk_col(t.grp, 0), bjj = 0;
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
        double xv[TC];   // first the shared -c [- tau*phi], then side 1's candidate
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {   // side 0, as k_du_rows
            const double aj = __shfl(al, jj), qj = __shfl(ql, jj);
            typename CS::Col ccol;
            cs.col_of_lane(ccol, clane, jj);
            double v = -cs.value(cr[jj], crow, ccol);
            if (a.cls2) {
                const double tf = tau * fr[jj];
                v = v - tf;
            }
            xv[jj] = v;
            const double pa = pi * aj;
            v = v - pa;
            v = v / qj;
            const double cand = (j0 + jj < g.n && v == v) ? v : -INFINITY;   // a NaN never wins
            if (cand > bv) {   // columns ascend: the first of equal maxima stays
                bv = cand;
                bj0 = j0;
                bjj = jj;
            }
        }
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {   // side 1, as k_du_cols
            const double qj = __shfl(ql, jj);
            const double qb = qj * bi;
            double v = xv[jj] - qb;
            v = v / pi;
            xv[jj] = (t.in_i && j0 + jj < g.n && v == v) ? v : -INFINITY;
        }
        double mv;
        int mi, col;
        colmax16(xv, t.in_i ? t.i : DU_NOIDX, t.lane, mv, mi);
        if (walk_col_owner(t, g, j0, col)) {
            const size_t at = walk_row_part_len(g) + walk_col_part_index(g, slot, col);   // du_part_index of side 1
            a.pv[at] = mv;
            a.pi[at] = mi;
        }
    }
    if (t.in_i) {
        a.pv[walk_row_part_index(g, t.grp, t.i)] = bv;   // du_part_index of side 0
        a.pi[walk_row_part_index(g, t.grp, t.i)] = bj0 + bjj;
    }
}

struct DuEval2 {
    DuGeo g;
    int cls2;
    const double* c;      // CostStored
    const double* phi;    // class 2
    const double* p;
    const double* q;
    const double* lam0;   // the two multipliers
    const double* lam1;
    const double* x;
    DuEvalPart* part0;    // walk_block_index
    DuEvalPart* part1;
};

// k_du_eval<true> for two multipliers at once (never with finite gama: cap stays 0, as there)
template <class CS>
__global__ __launch_bounds__(256) void k_du_eval2(const DuEval2 a, const CS cs) {
    __shared__ DuEvalPart red0[APD_WAVES], red1[APD_WAVES];
    const DuGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const double pi = a.p[t.ic];
    const double bi0 = a.lam0[g.n + t.ic], bi1 = a.lam1[g.n + t.ic];
    const double tau0 = a.cls2 ? a.lam0[g.n + g.m] : 0.0, tau1 = a.cls2 ? a.lam1[g.n + g.m] : 0.0;
    typename CS::Row crow;
    cs.row(crow, t.ic);
    double dmin0 = INFINITY, dmin1 = INFINITY, fv = 0.0;
    long long didx0 = DU_NOPLACE, didx1 = DU_NOPLACE;
    int nneg0 = 0, nneg1 = 0;
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        double cr[TC], fr[TC], xr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const size_t idx = walk_place(t, g, j0, jj);
            cr[jj] = CS::FREE ? 0.0 : a.c[idx];
            xr[jj] = a.x[idx];
            fr[jj] = a.cls2 ? a.phi[idx] : 0.0;
        }
        const int jl = walk_lane_col(t, g, j0);
        const double al0 = a.lam0[jl], al1 = a.lam1[jl];
        const double ql = a.q[jl];
        typename CS::Col clane;
        cs.col(clane, jl);
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const double aj0 = __shfl(al0, jj), aj1 = __shfl(al1, jj), qj = __shfl(ql, jj);
            typename CS::Col ccol;
            cs.col_of_lane(ccol, clane, jj);
            const double cv = cs.value(cr[jj], crow, ccol);
            const double pa0 = pi * aj0, pa1 = pi * aj1;
            double d0 = cv + pa0, d1 = cv + pa1;
            const double qb0 = qj * bi0, qb1 = qj * bi1;
            d0 = d0 + qb0;
            d1 = d1 + qb1;
            if (a.cls2) {
                const double tf0 = tau0 * fr[jj], tf1 = tau1 * fr[jj];
                d0 = d0 + tf0;
                d1 = d1 + tf1;
            }
            const bool valid = t.in_i && j0 + jj < g.n;
            const long long place = (long long)(j0 + jj) * g.m + t.i;
            if (valid && d0 < dmin0) {   // columns ascend: the first of equal minima stays; a NaN never wins
                dmin0 = d0;
                didx0 = place;
            }
            if (valid && d1 < dmin1) {
                dmin1 = d1;
                didx1 = place;
            }
            nneg0 += (valid && d0 < 0.0) ? 1 : 0;
            nneg1 += (valid && d1 < 0.0) ? 1 : 0;
            const double cx = cv * xr[jj];
            fv += valid ? cx : 0.0;
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        du_merge_min(dmin0, didx0, __shfl_xor(dmin0, s), __shfl_xor(didx0, s));
        du_merge_min(dmin1, didx1, __shfl_xor(dmin1, s), __shfl_xor(didx1, s));
        nneg0 += __shfl_xor(nneg0, s);
        nneg1 += __shfl_xor(nneg1, s);
    }
    fv = wave_sum(fv);
    if (t.lane == 0) {
        red0[t.wv].dmin = dmin0;
        red0[t.wv].idx = didx0;
        red0[t.wv].nneg = nneg0;
        red0[t.wv].cap = 0.0;
        red0[t.wv].fval = fv;
        red1[t.wv].dmin = dmin1;
        red1[t.wv].idx = didx1;
        red1[t.wv].nneg = nneg1;
        red1[t.wv].cap = 0.0;
        red1[t.wv].fval = fv;
    }
    __syncthreads();
    if (t.tid < 2) {   // thread 0 the first multiplier's, thread 1 the second's
        const DuEvalPart* red = t.tid ? red1 : red0;
        DuEvalPart r = red[0];
#pragma unroll
        for (int w = 1; w < APD_WAVES; ++w) {
            du_merge_min(r.dmin, r.idx, red[w].dmin, red[w].idx);
            r.nneg += red[w].nneg;
            r.fval += red[w].fval;
        }
        (t.tid ? a.part1 : a.part0)[walk_block_index(g, t.ib, t.grp)] = r;
    }
}

// what lies together in the scratch and comes back in one fetch
struct BracketStats {
    double dual[2][APD_STATS_DOUBLES];
    double round[2][APD_STATS_DOUBLES];
    NwInfoDev nw[2];   // read back under a correction mode other than 0 only
};

void check_args(const ipd_apd* h, double tol, int32_t install, const ipd_bracket* out) {
    IPD_REQUIRE(h && out, IPD_E_ARG, "ipd_apd_bracket: NULL argument");
    apd_round_check_args(h, tol, install);   // tol, install; finite gama is IPD_E_UNSUPPORTED
}

// the body of the two entries: `give` hands the winner's vectors to the caller
template <class Give>
void bracket_call(ipd_apd* h, double tol, int32_t install, ipd_bracket* out, Give&& give) {
    check_args(h, tol, install, out);
    ipd_ctx* ctx = h->ctx;
    CallScope scope(ctx);
    apd_dual_check_divider(h, 0);
    apd_dual_check_divider(h, 1);
    const BracketRun r = apd_bracket_measure(h, tol);
    IPD_REQUIRE(!install || r.b.upper.ok, IPD_E_NUMERIC,
                "ipd_apd_bracket: no repair of this shape exists (ok = 0); nothing was installed");
    if (install) apd_bracket_install(h, r);
    give(r);
    ctx->sync();   // the scratch arrays are the next call's
    *out = r.b;
}

}  // namespace

BracketRun apd_bracket_measure(ipd_apd* h, double tol) {
    ipd_ctx* ctx = h->ctx;
    Arena& S = *ctx->scratch;
    const DuGeo g0 = du_make_geo(h->m, h->n, 0), g1 = du_make_geo(h->m, h->n, 1);
    const dim3 grid(g0.nib, g0.ng);
    const int cls2 = h->cls == 2 ? 1 : 0;
    const size_t L = (size_t)h->L;
    const size_t part_doubles = (size_t)walk_blocks(g0) * (sizeof(DuEvalPart) / sizeof(double));
    BracketStats* st = reinterpret_cast<BracketStats*>(S.alloc<double>(sizeof(BracketStats) / sizeof(double)));
    BracketRun r;
    r.tol = tol;
    // the lower side
    DuBoth a;
    a.g = g0;
    a.cls2 = cls2;
    a.c = h->c;
    a.phi = h->phi;
    a.p = h->p;
    a.q = h->q;
    a.lam = h->lam;
    a.pv = S.alloc<double>(du_part_len(g0) + du_part_len(g1));
    a.pi = S.alloc<int>(du_part_len(g0) + du_part_len(g1));
    with_cost_source(h, [&](auto cs) {
        hipLaunchKernelGGL((k_du_both<decltype(cs)>), grid, dim3(256), 0, ctx->stream, a, cs);
    });
    IPD_KERNEL_CHECK();
    double* lam0 = S.alloc<double>(L);
    double* lam1 = S.alloc<double>(L);
    apd_dual_finish(h, 0, a.pv, a.pi, h->lam, lam0, nullptr);
    apd_dual_finish(h, 1, a.pv + du_part_len(g0), a.pi + du_part_len(g0), h->lam, lam1, nullptr);
    DuEval2 e;
    e.g = g0;
    e.cls2 = cls2;
    e.c = h->c;
    e.phi = h->phi;
    e.p = h->p;
    e.q = h->q;
    e.lam0 = lam0;
    e.lam1 = lam1;
    e.x = h->u;   // class 2: the x block of uk comes first
    e.part0 = reinterpret_cast<DuEvalPart*>(S.alloc<double>(part_doubles));
    e.part1 = reinterpret_cast<DuEvalPart*>(S.alloc<double>(part_doubles));
    with_cost_source(h, [&](auto cs) {
        hipLaunchKernelGGL((k_du_eval2<decltype(cs)>), grid, dim3(256), 0, ctx->stream, e, cs);
    });
    IPD_KERNEL_CHECK();
    apd_dual_last(h, e.part0, lam0, 1, reinterpret_cast<ipd_dual_stats*>(st->dual[0]));
    apd_dual_last(h, e.part1, lam1, 1, reinterpret_cast<ipd_dual_stats*>(st->dual[1]));
    r.lam[0] = lam0;
    r.lam[1] = lam1;
    // the upper side: pass A once, both first scale vectors out of its partials, then the rest of each side
    r.shared = apd_round_pass_a(h, tol);
    for (int s = 0; s < 2; ++s)
        r.side[s] = apd_round_first_scale(h, r.shared, s, reinterpret_cast<ipd_round_stats*>(st->round[s]), &st->nw[s]);
    for (int s = 0; s < 2; ++s) apd_round_rest(h, r.shared, r.side[s], tol);
    BracketStats got;
    ctx->fetch_bytes(st, &got, h->corr_mode != 0 ? sizeof(BracketStats) : offsetof(BracketStats, nw));
    ipd_dual_stats du[2];
    ipd_round_stats rd[2];
    for (int s = 0; s < 2; ++s) {
        std::memcpy(&du[s], got.dual[s], sizeof(ipd_dual_stats));
        std::memcpy(&rd[s], got.round[s], sizeof(ipd_round_stats));
    }
    r.b.lower_side = apd_gap_lower_side(du[0].dual, du[1].dual);
    r.b.upper_side = apd_gap_upper_side(rd[0].ok, rd[0].fval, rd[1].ok, rd[1].fval);
    r.b.lower = du[r.b.lower_side];
    r.b.upper = rd[r.b.upper_side];
    r.b.gap = apd_gap_value(r.b.upper.fval, r.b.lower.dual);
    apd_nw_record(h, r.b.upper_side, h->corr_mode != 0 ? &got.nw[r.b.upper_side] : nullptr);
    return r;
}
static_assert(sizeof(ipd_dual_stats) <= APD_STATS_DOUBLES * sizeof(double) &&
                  sizeof(ipd_round_stats) <= APD_STATS_DOUBLES * sizeof(double) &&
                  sizeof(DuEvalPart) % sizeof(double) == 0,
              "apd_bracket_measure sizes the results and the partials in doubles");

void apd_bracket_install(ipd_apd* h, const BracketRun& r) {
    apd_round_write(h, r.shared, r.side[r.b.upper_side], r.tol, 1, nullptr);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_bracket_dev(ipd_apd* h, double tol, int32_t install, double* lam_out_dev, double* rho_dev,
                                   double* kappa_dev, double* e_dev, double* f_dev, ipd_bracket* out) {
    return ipd_guard([&] {
        bracket_call(h, tol, install, out, [&](const BracketRun& r) {
            const RoundSide& v = r.side[r.b.upper_side];
            const size_t n = (size_t)h->n, m = (size_t)h->m;
            if (lam_out_dev) copy_dev(h, lam_out_dev, r.lam[r.b.lower_side], (size_t)h->L);
            if (rho_dev) copy_dev(h, rho_dev, v.sc + n, m);
            if (kappa_dev) copy_dev(h, kappa_dev, v.sc, n);
            if (e_dev) copy_dev(h, e_dev, v.ef + n, m);
            if (f_dev) copy_dev(h, f_dev, v.ef, n);
        });
    });
}

extern "C" int ipd_apd_bracket(ipd_apd* h, double tol, int32_t install, double* lam_out, double* rho, double* kappa,
                               double* e, double* f, ipd_bracket* out) {
    return ipd_guard([&] {
        bracket_call(h, tol, install, out, [&](const BracketRun& r) {
            ipd_ctx* ctx = h->ctx;
            const RoundSide& v = r.side[r.b.upper_side];
            const size_t n = (size_t)h->n, m = (size_t)h->m;
            if (lam_out) ctx->fetch(r.lam[r.b.lower_side], lam_out, (size_t)h->L);
            if (rho) ctx->fetch(v.sc + n, rho, m);
            if (kappa) ctx->fetch(v.sc, kappa, n);
            if (e) ctx->fetch(v.ef + n, e, m);
            if (f) ctx->fetch(v.ef, f, n);
        });
    });
}
