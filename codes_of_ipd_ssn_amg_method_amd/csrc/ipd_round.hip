// The primal certificate where the iterate lives (ipd_apd_round, ipd_apd_round_dev): the
// x block of the workspace's u rounded onto the transport polytope -- clamp, two scalings, a rank-one correction
// (Altschuler, Weed, Rigollet, Algorithm 2, with the weights p, q and class 2's phi row) -- and the exact cost of the
// result.  The result stays factored (rho, kappa, e, f, theta, t), so nothing mn-sized crosses the host boundary;
// partials and vectors live in the context's scratch arena, and the workspace is written only with install = 1.
//
//   walk   every mn-sized pass is one instantiation of k_rd_walk on the column-group walk of DESIGN.md section 4j
//          (ipd_walk_geo.h, ipd_walk_dev.h).  Row sums stay in a register over the column group (columns ascending) and
//          leave as one partial per (group, row); the 16 column sums of a chunk come out of colsum16's butterfly, one
//          partial per (segment slot, column); a scalar sum is a lane's sum over its entries (columns ascending), then
//          walk_wave_sums' shape, one partial per workgroup.  The kernel writes the frame of ipd_walk_dev.h out: taken
//          from there, passes D and W compile to other machine code.
//            A   x                  a0, b0 partials; dropped, ndropped
//            B   x                  side 0: b1 partials; side 1: a1 partials
//            C   x, c (, phi)       a2, b2 partials; fs (, ms)
//            D   c (, phi)          cc (, cp) -- reads nothing mn-sized on a matrix-free class-1 workspace
//            W   x                  X^ to up to three destinations (x_out, and with install the x blocks of u and v)
//   finish one thread per entry of [columns (n); rows (m)]: the partials of a column (slot ascending) or a row (group
//          ascending) in index order, sum_strided's bursts; then the scale or the deficit of that entry.
//   last   one workgroup: the scalars of A, C and D (thread t adds workgroups t, t + 256, ... in order, wave_sum's
//          tree, the four waves in order), Se, Sf and viol_in the same way over the rows resp. columns, then theta, t,
//          fval and ok on the device -- class 2's branch is taken there, D ran unconditionally.
//   slack  class 2 with install: y^, z^ into the y and z blocks of u and v.
// W and slack read ok from the device and write nothing when install was asked and ok = 0: the host learns of it
// from the one read-back of the statistics.
//
// The host side is four stages (ipd_apd_state.h: apd_round_pass_a, apd_round_first_scale, apd_round_rest,
// apd_round_write): a call here runs them for one side, ipd_bracket.hip runs pass A once for both sides.
//
// Geometry and every index: ipd_round_geo.h.  Deterministic: every sum has a fixed shape, no float atomics -- two
// calls give the same bits, and so do the host and the device entry and the three cost sources.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>
#include <limits>

#include "ipd_apd_state.h"
#include "ipd_round_geo.h"
#include "ipd_walk_dev.h"

namespace {

enum { RD_A = 0, RD_B0 = 1, RD_B1 = 2, RD_C = 3, RD_D = 4, RD_W = 5 };

// (RdDev, what the last kernel leaves on the device for W and slack: ipd_apd_state.h)
static_assert(sizeof(ipd_round_stats) <= APD_STATS_DOUBLES * sizeof(double) && sizeof(RdDev) <= 8 * sizeof(double) &&
                  RD_RESULT_DOUBLES == 24,
              "round_dev sizes the result in doubles");

// step 1: plan()'s threshold, then the clamp at 0; a NaN becomes 0
__device__ __forceinline__ double rd_clamp(double x, double tol) {
    return (walk_keep(x, tol) && x > 0.0) ? x : 0.0;
}
__device__ __forceinline__ double rd_scale(double s, double bound) { return s > bound ? bound / s : 1.0; }

// the cost source CS of a pass that reads c (CostStored or CostFree<D>, ipd_apd_tiles.h) is an argument of its own
struct RdWalk {
    RdGeo g;
    int cls2;
    int need_ok;         // W: write only when dev->ok
    double tol;
    const double* x;     // the x block of u
    const double* c;     // CostStored
    const double* phi;   // class 2
    const double* p;
    const double* q;
    const double* sc;    // [kappa (n); rho (m)]
    const double* ef;    // [f (n); e (m)]
    const RdDev* dev;    // W
    double* rpart;       // walk_row_part_index
    double* cpart;       // walk_col_part_index
    double* spart;       // rd_scal_index
    double* o0;          // W: destinations or nullptr
    double* o1;
    double* o2;
};

template <int PASS, class CS>
__global__ __launch_bounds__(256) void k_rd_walk(const RdWalk a, const CS cs) {
    constexpr bool USE_X = PASS != RD_D;
    constexpr bool USE_C = PASS == RD_C || PASS == RD_D;
    constexpr bool ROWS = PASS == RD_A || PASS == RD_B1 || PASS == RD_C;
    constexpr bool COLS = PASS == RD_A || PASS == RD_B0 || PASS == RD_C;
    constexpr bool SCAL = PASS == RD_A || PASS == RD_C || PASS == RD_D;
    constexpr bool USE_RHO = PASS == RD_B0 || PASS == RD_C || PASS == RD_W;
    constexpr bool USE_KAP = PASS == RD_B1 || PASS == RD_C || PASS == RD_W;
    constexpr bool USE_EF = PASS == RD_D || PASS == RD_W;
    __shared__ double red[APD_WAVES * RD_NS];
    const RdGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;   // walk_lane
    const int ib = blockIdx.x, grp = blockIdx.y;
    const int i = ib * TR + tid;
    const bool in_i = i < g.m;
    const int ic = in_i ? i : g.m - 1;
    double theta = 1.0, tt = 0.0;
    if (PASS == RD_W) {
        if (a.need_ok && !a.dev->ok) return;   // uniform; this pass has no barrier
        theta = a.dev->theta;
        tt = a.dev->t;
    }
    const double pi = a.p[ic];
    const double rho = USE_RHO ? a.sc[g.n + ic] : 1.0;
    const double ei = USE_EF ? a.ef[g.n + ic] : 0.0;
    typename CS::Row crow;
    if (USE_C) cs.row(crow, ic);
    double racc = 0.0, s0 = 0.0, s1 = 0.0;
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(grp, ch);
        if (j0 >= g.n) break;  // uniform
        double xr[TC], cr[TC], fr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const int j = min(j0 + jj, g.n - 1);   // walk_place
            const size_t idx = (size_t)j * g.m + ic;
            xr[jj] = USE_X ? a.x[idx] : 0.0;
            cr[jj] = (USE_C && !CS::FREE) ? a.c[idx] : 0.0;
            fr[jj] = (USE_C && a.cls2) ? a.phi[idx] : 0.0;
        }
        const int jl = min(j0 + (lane & (TC - 1)), g.n - 1);   // walk_lane_col
        const double ql = ROWS ? a.q[jl] : 0.0;
        const double kl = USE_KAP ? a.sc[jl] : 1.0;
        const double fl = USE_EF ? a.ef[jl] : 0.0;
        typename CS::Col clane;
        if (USE_C) cs.col(clane, jl);
        double xv[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const bool valid = in_i && j0 + jj < g.n;
            const double qj = ROWS ? __shfl(ql, jj) : 0.0;
            const double kj = USE_KAP ? __shfl(kl, jj) : 1.0;
            const double fj = USE_EF ? __shfl(fl, jj) : 0.0;
            double cv = 0.0;
            if (USE_C) {
                typename CS::Col ccol;
                cs.col_of_lane(ccol, clane, jj);
                cv = cs.value(cr[jj], crow, ccol);
            }
            const double xp = USE_X ? rd_clamp(xr[jj], a.tol) : 0.0;
            double term_r = 0.0, term_c = 0.0;
            if (PASS == RD_A) {
                term_r = qj * xp;
                term_c = pi * xp;
                const bool drop = valid && xr[jj] != 0.0 && xp == 0.0;   // a NaN is counted and adds nothing
                const double ax = fabs(xr[jj]);
                s0 += (drop && ax == ax) ? ax : 0.0;
                s1 += drop ? 1.0 : 0.0;
            } else if (PASS == RD_B0) {
                const double y = rho * xp;
                term_c = pi * y;
            } else if (PASS == RD_B1) {
                const double y = xp * kj;
                term_r = qj * y;
            } else if (PASS == RD_C) {
                const double y = rho * xp;
                const double x2 = y * kj;
                term_r = qj * x2;
                term_c = pi * x2;
                const double w0 = cv * x2;
                s0 += valid ? w0 : 0.0;
                if (a.cls2) {
                    const double w1 = fr[jj] * x2;
                    s1 += valid ? w1 : 0.0;
                }
            } else if (PASS == RD_D) {
                const double efv = ei * fj;
                const double w0 = cv * efv;
                s0 += valid ? w0 : 0.0;
                if (a.cls2) {
                    const double w1 = fr[jj] * efv;
                    s1 += valid ? w1 : 0.0;
                }
            } else {   // RD_W
                const double y = rho * xp;
                const double x2 = y * kj;
                const double efv = ei * fj;
                const double t1 = theta * x2;
                const double t2 = tt * efv;
                const double xh = t1 + t2;
                if (valid) {
                    const size_t idx = (size_t)(j0 + jj) * g.m + i;
                    if (a.o0) a.o0[idx] = xh;
                    if (a.o1) a.o1[idx] = xh;
                    if (a.o2) a.o2[idx] = xh;
                }
            }
            if (ROWS) racc += valid ? term_r : 0.0;
            xv[jj] = valid ? term_c : 0.0;
        }
        if (COLS) {
            const double cs = colsum16(xv, lane);
            const int col = j0 + colsum_index(lane);
            if (lane < 16 && col < g.n) a.cpart[walk_col_part_index(g, walk_slot(ib, wv), col)] = cs;
        }
    }
    if (ROWS && in_i) a.rpart[walk_row_part_index(g, grp, i)] = racc;
    if (SCAL) {
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            red[wv * RD_NS + 0] = s0;
            red[wv * RD_NS + 1] = s1;
        }
        __syncthreads();
        if (tid < RD_NS) {
            double r = red[tid];
#pragma unroll
            for (int w = 1; w < APD_WAVES; ++w) r += red[w * RD_NS + tid];
            a.spart[rd_scal_index(g, ib, grp, tid)] = r;
        }
    }
}

// ---------------------------------------------------------------------------
// finish: one thread per entry of [columns (n); rows (m)]
// ---------------------------------------------------------------------------
struct RdFin {
    RdGeo g;
    int side;
    const double* rpart;
    const double* cpart;
    const double* b;     // [r (n); l (m)(; mu)]
    double* ab0;         // [b0; a0]
    double* sc;          // [kappa; rho]
    double* ab2;         // [b2; a2]
    double* ef;          // [f; e]
};

// STEP 0: after A (first marginals, the first scale vector); 1: after B (the second scale vector); 2: after C (the
// marginals of the scaled plan, the deficits)
template <int STEP>
__global__ __launch_bounds__(256) void k_rd_fin(const RdFin a) {
    const RdGeo& g = a.g;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.n + g.m) return;
    const bool col = t < g.n;
    const bool first = col ? a.side == 1 : a.side == 0;   // is this entry's scale the first of the two?
    if (STEP == 1 && first) return;
    const double s = col ? sum_strided(a.cpart + t, g.nslot, (size_t)g.n)
                         : sum_strided(a.rpart + (t - g.n), g.ng, (size_t)g.m);
    const double bt = a.b[t];
    if (STEP == 0) {
        a.ab0[t] = s;
        if (first) a.sc[t] = rd_scale(s, bt);
    } else if (STEP == 1) {
        a.sc[t] = rd_scale(s, bt);
    } else {
        a.ab2[t] = s;
        const double d = bt - s;
        a.ef[t] = walk_pos(d);
    }
}

// ---------------------------------------------------------------------------
// last
// ---------------------------------------------------------------------------
struct RdLast {
    RdGeo g;
    int cls2;
    double mu;
    const double* sA;    // the scalars of A, C, D: rd_scal_index
    const double* sC;
    const double* sD;
    const double* ab0;
    const double* ef;
    const double* b;
    const double* p;
    const double* q;
    ipd_round_stats* out;
    RdDev* dev;
};

constexpr int RD_NSUM = 10;

__global__ __launch_bounds__(256) void k_rd_last(const RdLast a) {
    __shared__ double red[APD_WAVES * RD_NSUM];
    const RdGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int nblk = walk_blocks(g);
    // 0 dropped, 1 ndropped, 2 fs, 3 ms, 4 cc, 5 cp, 6 Se, 7 the rows of viol_in, 8 Sf, 9 the columns of viol_in
    double s[RD_NSUM];
#pragma unroll
    for (int k = 0; k < RD_NSUM; ++k) s[k] = 0.0;
#pragma unroll 4
    for (int k = tid; k < nblk; k += 256) {
        s[0] += a.sA[(size_t)k * RD_NS + 0];
        s[1] += a.sA[(size_t)k * RD_NS + 1];
        s[2] += a.sC[(size_t)k * RD_NS + 0];
        s[3] += a.sC[(size_t)k * RD_NS + 1];
        s[4] += a.sD[(size_t)k * RD_NS + 0];
        s[5] += a.sD[(size_t)k * RD_NS + 1];
    }
#pragma unroll 4
    for (int i = tid; i < g.m; i += 256) {
        const double pi = a.p[i];
        const double pe = pi * a.ef[g.n + i];
        s[6] += pe;
        const double d = a.ab0[g.n + i] - a.b[g.n + i];
        const double v = a.cls2 ? walk_pos(d) : fabs(d);
        const double pv = pi * v;
        s[7] += pv;
    }
#pragma unroll 4
    for (int j = tid; j < g.n; j += 256) {
        const double qj = a.q[j];
        const double qf = qj * a.ef[j];
        s[8] += qf;
        const double d = a.ab0[j] - a.b[j];
        const double v = a.cls2 ? walk_pos(d) : fabs(d);
        const double qv = qj * v;
        s[9] += qv;
    }
    walk_wave_sums(lane, wv, s, red);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < RD_NSUM; ++k) s[k] = walk_waves_total<RD_NSUM>(red, k);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const double fs = s[2], ms = s[3], cc = s[4], cp = s[5], se = s[6], sf = s[8];
        double theta = 1.0, t;
        if (!a.cls2) {
            t = se > 0.0 ? 1.0 / se : 0.0;
        } else if (ms >= a.mu) {
            theta = a.mu / ms;
            t = 0.0;
        } else {
            const double d = a.mu - ms;
            t = d / cp;
        }
        const double f1 = theta * fs;
        const double f2 = t * cc;
        const double fval = f1 + f2;
        bool ok = isfinite(theta) && isfinite(t) && isfinite(fval);
        if (a.cls2) {
            const double ts = t * se, tf = t * sf;
            ok = ok && ts <= 1.0 && tf <= 1.0;
        }
        ipd_round_stats st = {};
        st.fval = fval;
        st.fs = fs;
        st.cc = cc;
        st.theta = theta;
        st.t = t;
        st.se = se;
        st.sf = sf;
        st.ms = a.cls2 ? ms : nan;
        st.cp = a.cls2 ? cp : nan;
        st.viol_in = s[7] + s[9];
        st.dropped = s[0];
        st.ndropped = (int64_t)s[1];
        st.ok = ok ? 1 : 0;
        *a.out = st;
        RdDev dv;
        dv.theta = theta;
        dv.t = t;
        dv.se = se;
        dv.sf = sf;
        dv.ok = ok ? 1 : 0;
        *a.dev = dv;
    }
}

// class 2 with install: y^_j = max(r_j - (theta*b2_j + t*(Se*f_j)), 0), z^_i = max(l_i - (theta*a2_i + t*(e_i*Sf)), 0)
struct RdSlack {
    RdGeo g;
    const RdDev* dev;
    const double* ab2;
    const double* ef;
    const double* b;
    double* u_yz;   // the y and z blocks of u: n + m entries
    double* v_yz;
};

__global__ __launch_bounds__(256) void k_rd_slack(const RdSlack a) {
    const RdGeo& g = a.g;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= g.n + g.m || !a.dev->ok) return;
    const double theta = a.dev->theta, tt = a.dev->t;
    const double ev = a.ef[t];
    const double w = t < g.n ? a.dev->se * ev : ev * a.dev->sf;
    const double t1 = theta * a.ab2[t];
    const double t2 = tt * w;
    const double v = t1 + t2;
    const double d = a.b[t] - v;
    const double y = walk_pos(d);
    a.u_yz[t] = y;
    a.v_yz[t] = y;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int PASS, class CS = CostStored>
void launch_walk(ipd_apd* h, const RdWalk& a, CS cs = CS()) {
    hipLaunchKernelGGL((k_rd_walk<PASS, CS>), dim3(a.g.nib, a.g.ng), dim3(256), 0, h->ctx->stream, a, cs);
    IPD_KERNEL_CHECK();
}

RdWalk walk_args(ipd_apd* h, const RoundShared& sh, const RoundSide& s, double tol) {
    RdWalk w;
    w.g = walk_make_geo(h->m, h->n);
    w.cls2 = h->cls == 2 ? 1 : 0;
    w.need_ok = 0;
    w.tol = tol;
    w.x = h->u;   // class 2: the x block of uk comes first
    w.c = h->c;
    w.phi = h->phi;
    w.p = h->p;
    w.q = h->q;
    w.sc = s.sc;
    w.ef = s.ef;
    w.dev = static_cast<const RdDev*>(s.dev);
    w.rpart = sh.rpart;
    w.cpart = sh.cpart;
    w.spart = sh.sA;
    w.o0 = w.o1 = w.o2 = nullptr;
    return w;
}

RdFin fin_args(ipd_apd* h, const RoundShared& sh, const RoundSide& s) {
    RdFin f;
    f.g = walk_make_geo(h->m, h->n);
    f.side = s.side;
    f.rpart = sh.rpart;
    f.cpart = sh.cpart;
    f.b = h->b;
    f.ab0 = sh.ab0;
    f.sc = s.sc;
    f.ab2 = s.ab2;
    f.ef = s.ef;
    return f;
}

dim3 fin_grid(const ipd_apd* h) { return dim3(cdiv((long long)h->M, 256)); }

}  // namespace

// pass A: the first marginals' partials and the scalars of the clamp, shared by the two sides
RoundShared apd_round_pass_a(ipd_apd* h, double tol) {
    Arena& S = *h->ctx->scratch;
    const RdGeo g = walk_make_geo(h->m, h->n);
    RoundShared sh;
    sh.rpart = S.alloc<double>(walk_row_part_len(g));
    sh.cpart = S.alloc<double>(walk_col_part_len(g));
    sh.sA = S.alloc<double>(rd_scal_len(g));
    sh.ab0 = S.alloc<double>((size_t)h->M);
    launch_walk<RD_A>(h, walk_args(h, sh, RoundSide{}, tol));
    return sh;
}

// one side's arrays and its first scale vector out of pass A's partials, which the rest of a side overwrites
RoundSide apd_round_first_scale(ipd_apd* h, const RoundShared& sh, int side, ipd_round_stats* out_dev,
                                NwInfoDev* info_dev) {
    Arena& S = *h->ctx->scratch;
    const RdGeo g = walk_make_geo(h->m, h->n);
    const size_t M = (size_t)h->M;
    RoundSide s;
    s.side = side;
    s.sC = S.alloc<double>(rd_scal_len(g));
    s.sD = S.alloc<double>(rd_scal_len(g));
    s.sc = S.alloc<double>(M);
    s.ab2 = S.alloc<double>(M);
    s.ef = S.alloc<double>(M);
    s.out = out_dev ? out_dev : reinterpret_cast<ipd_round_stats*>(S.alloc<double>(APD_STATS_DOUBLES));
    s.dev = S.alloc<double>(8);
    if (h->corr_mode != 0) s.nw = apd_nw_side(h, side, info_dev);
    hipLaunchKernelGGL(k_rd_fin<0>, fin_grid(h), dim3(256), 0, h->ctx->stream, fin_args(h, sh, s));
    IPD_KERNEL_CHECK();
    return s;
}

// B, C, D with their finishing kernels and the last kernel: s.out and s.dev are complete on the stream afterwards.
// Mode 1 of the correction runs no pass D, and modes 1 and 2 end in ipd_round_nw.hip's kernels.
void apd_round_rest(ipd_apd* h, const RoundShared& sh, const RoundSide& s, double tol) {
    ipd_ctx* ctx = h->ctx;
    RdWalk w = walk_args(h, sh, s, tol);
    const RdFin f = fin_args(h, sh, s);
    if (s.side == 0)
        launch_walk<RD_B0>(h, w);
    else
        launch_walk<RD_B1>(h, w);
    hipLaunchKernelGGL(k_rd_fin<1>, fin_grid(h), dim3(256), 0, ctx->stream, f);
    IPD_KERNEL_CHECK();
    w.spart = s.sC;
    with_cost_source(h, [&](auto cs) { launch_walk<RD_C>(h, w, cs); });
    hipLaunchKernelGGL(k_rd_fin<2>, fin_grid(h), dim3(256), 0, ctx->stream, f);
    IPD_KERNEL_CHECK();
    w.spart = s.sD;
    if (h->corr_mode != 1) with_cost_source(h, [&](auto cs) { launch_walk<RD_D>(h, w, cs); });
    if (h->corr_mode != 0) return apd_nw_rest(h, sh, s);
    RdLast l;
    l.g = w.g;
    l.cls2 = w.cls2;
    l.mu = h->mu;
    l.sA = sh.sA;
    l.sC = s.sC;
    l.sD = s.sD;
    l.ab0 = sh.ab0;
    l.ef = s.ef;
    l.b = h->b;
    l.p = h->p;
    l.q = h->q;
    l.out = s.out;
    l.dev = static_cast<RdDev*>(s.dev);
    hipLaunchKernelGGL(k_rd_last, dim3(1), dim3(256), 0, ctx->stream, l);
    IPD_KERNEL_CHECK();
}

// X^ of a finished side to x_out_dev (or nullptr) and, with install, into the state (class 2: with its slacks); the
// kernels read ok from the device and write nothing when install was asked and ok = 0
void apd_round_write(ipd_apd* h, const RoundShared& sh, const RoundSide& s, double tol, int install,
                     double* x_out_dev) {
    if (!install && !x_out_dev) return;
    RdWalk w = walk_args(h, sh, s, tol);
    w.need_ok = install;
    w.o0 = x_out_dev;
    w.o1 = install ? h->u : nullptr;
    w.o2 = install ? h->v : nullptr;
    if (h->corr_mode != 0) w.dev = s.nw.devw;   // t = 0 there when the list carries the correction
    launch_walk<RD_W>(h, w);
    if (h->corr_mode != 0) apd_nw_scatter(h, s, install, w.o0, w.o1, w.o2);
    if (install && h->cls == 2) {
        RdSlack k;
        k.g = w.g;
        k.dev = static_cast<const RdDev*>(s.dev);
        k.ab2 = s.ab2;
        k.ef = s.ef;
        k.b = h->b;
        k.u_yz = h->u + h->mn;
        k.v_yz = h->v + h->mn;
        hipLaunchKernelGGL(k_rd_slack, fin_grid(h), dim3(256), 0, h->ctx->stream, k);
        IPD_KERNEL_CHECK();
    }
}

void apd_round_check_args(const ipd_apd* h, double tol, int32_t install) {
    IPD_REQUIRE(install == 0 || install == 1, IPD_E_ARG, "ipd_apd_round: install must be 0 or 1");
    IPD_REQUIRE(tol >= 0.0, IPD_E_ARG, "ipd_apd_round: tol must be >= 0");   // a NaN fails the comparison
    IPD_REQUIRE(!(h->cls == 1 && (h->gama || std::isfinite(h->P.gs))), IPD_E_UNSUPPORTED,
                "ipd_apd_round: the rank-one correction does not keep x <= gama; finite gama is not supported");
}

namespace {

void check_args(const ipd_apd* h, double tol, int32_t side, int32_t install, const ipd_round_stats* st) {
    IPD_REQUIRE(h && st, IPD_E_ARG, "ipd_apd_round: NULL argument");
    IPD_REQUIRE(side == 0 || side == 1, IPD_E_ARG, "ipd_apd_round: side must be 0 or 1");
    apd_round_check_args(h, tol, install);
}

// all launches of a call on the context's stream; *st is read back (the stream is waited for).  IPD_E_NUMERIC when
// install was asked and ok = 0: the device wrote nothing then.
RoundSide round_dev(ipd_apd* h, double tol, int side, int install, double* x_out_dev, ipd_round_stats* st) {
    const RoundShared sh = apd_round_pass_a(h, tol);
    // under a correction mode other than 0 the statistics and what the correction adds lie together: one read-back
    struct Both {
        double stats[APD_STATS_DOUBLES];
        NwInfoDev info;
    };
    Both* both = h->corr_mode == 0
                     ? nullptr
                     : reinterpret_cast<Both*>(h->ctx->scratch->alloc<double>(sizeof(Both) / sizeof(double)));
    const RoundSide s = apd_round_first_scale(h, sh, side, both ? reinterpret_cast<ipd_round_stats*>(both->stats) : nullptr,
                                              both ? &both->info : nullptr);
    apd_round_rest(h, sh, s, tol);
    apd_round_write(h, sh, s, tol, install, x_out_dev);
    if (both) {
        Both got;
        h->ctx->fetch_bytes(both, &got, sizeof(Both));
        std::memcpy(st, got.stats, sizeof(ipd_round_stats));
        apd_nw_record(h, side, &got.info);
    } else {
        h->ctx->fetch_bytes(s.out, st, sizeof(ipd_round_stats));
        apd_nw_record(h, side, nullptr);
    }
    if (install && !st->ok)
        throw IpdError(IPD_E_NUMERIC, "ipd_apd_round: no repair of this shape exists (ok = 0); nothing was installed");
    return s;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_round_dev(ipd_apd* h, double tol, int32_t side, int32_t install, double* rho_dev,
                                 double* kappa_dev, double* e_dev, double* f_dev, double* x_out_dev,
                                 ipd_round_stats* st) {
    return ipd_guard([&] {
        check_args(h, tol, side, install, st);
        CallScope scope(h->ctx);
        ipd_round_stats got;
        const RoundSide v = round_dev(h, tol, side, install, x_out_dev, &got);
        const size_t n = (size_t)h->n, m = (size_t)h->m;
        if (rho_dev) copy_dev(h, rho_dev, v.sc + n, m);
        if (kappa_dev) copy_dev(h, kappa_dev, v.sc, n);
        if (e_dev) copy_dev(h, e_dev, v.ef + n, m);
        if (f_dev) copy_dev(h, f_dev, v.ef, n);
        h->ctx->sync();   // the scratch arrays are the next call's
        *st = got;
    });
}

extern "C" int ipd_apd_round(ipd_apd* h, double tol, int32_t side, int32_t install, double* rho, double* kappa,
                             double* e, double* f, ipd_round_stats* st) {
    return ipd_guard([&] {
        check_args(h, tol, side, install, st);
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        ipd_round_stats got;
        const RoundSide v = round_dev(h, tol, side, install, nullptr, &got);
        const size_t n = (size_t)h->n, m = (size_t)h->m;
        if (rho) ctx->fetch(v.sc + n, rho, m);
        if (kappa) ctx->fetch(v.sc, kappa, n);
        if (e) ctx->fetch(v.ef + n, e, m);
        if (f) ctx->fetch(v.ef, f, n);
        ctx->sync();
        *st = got;
    });
}
