// The transport plan applied where it lives (ipd_apd_plan_apply, ipd_apd_plan_apply_dev):
// Y = X*B (side 0) or Y = X'*B (side 1) for a thin dense B of k <= 16 columns, X being what ipd_apd_plan would
// return at the same tol -- x(i,j) = u[i + j*m], kept when !(|x| <= tol) -- with the mass w = X*1 (X'*1) of the kept
// entries and, on request, the rows of Y divided by it (the barycentric projection).  Nothing mn-sized crosses the
// host boundary and nothing of the workspace is written: the partials live in the context's scratch arena.
//
//   walk    one streaming read of x per pass of PA_KC = 4 components, on the column-group walk of DESIGN.md section 4j
//           (ipd_walk_geo.h, ipd_walk_dev.h).  A dropped entry, a padding lane and a clamped column contribute +0.0
//           through a select, so an inf or NaN of B that meets only those never reaches Y.
//     side 0  lane l loads B[j0 + (l & 15), c0 + (l >> 4)], one load per lane and chunk.  KC row accumulators and the
//             mass stay in registers over the column group and leave as one partial per (group, component, row).
//     side 1  a lane holds B(i, c0 .. c0+KC) in registers; per chunk and component one colsum16 butterfly gives the
//             wave's 16 column sums, one partial per (segment slot, component, column).
//   finish  one thread per entry of the pass's columns of Y adds its partials in index order, divides by the mass
//           when asked to (one IEEE division; a row of zero kept mass is 0/0 = NaN) and stores.  Pass 0 also sums the
//           mass and leaves it in w (the caller's, or a scratch vector) for the passes after it.
//
// Geometry, pass split and every index: ipd_plan_apply_geo.h.  Deterministic: every sum has a fixed shape, no float
// atomics -- two calls give the same bits, and so do the host and the device entry.
#pragma clang fp contract(off)

#include <cmath>

#include "ipd_apd_state.h"
#include "ipd_plan_apply_geo.h"
#include "ipd_walk_dev.h"

namespace {

// TR, TC: ipd_apd_geo.h; colsum16, sum_strided: ipd_apd_tiles.h
static_assert(PA_KC * TC == 64, "side 0: the lanes of a wave fetch a chunk's TC x PA_KC block of B in one load each");

struct PaWalk {
    PaGeo g;
    int c0;            // first component of the pass
    const double* x;
    const double* B;
    double tol;
    double* part;      // pa_part_index
};

// ---------------------------------------------------------------------------
// side 0: Y = X*B
// ---------------------------------------------------------------------------
template <int KC, bool MASS>
__global__ __launch_bounds__(256) void k_pa_rows(const PaWalk a) {
    const PaGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    double acc[KC], wacc = 0.0;
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[c] = 0.0;
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        double xr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) xr[jj] = a.x[walk_place(t, g, j0, jj)];
        // lane l fetches B(j0 + (l & 15), c0 + (l >> 4))
        const int lc = t.lane >> 4;
        const double bl = lc < KC ? a.B[(size_t)(a.c0 + lc) * g.n + walk_lane_col(t, g, j0)] : 0.0;
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const double x = xr[jj];
            const bool keep = t.in_i && j0 + jj < g.n && walk_keep(x, a.tol);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const double b = __shfl(bl, c * TC + jj);
                const double xb = x * b;
                acc[c] += keep ? xb : 0.0;
            }
            if (MASS) wacc += keep ? x : 0.0;
        }
    }
    if (t.in_i) {
#pragma unroll
        for (int c = 0; c < KC; ++c) a.part[pa_part_index(g, t.grp, c, t.i)] = acc[c];
        if (MASS) a.part[pa_part_index(g, t.grp, PA_KC, t.i)] = wacc;
    }
}

// ---------------------------------------------------------------------------
// side 1: Y = X'*B
// ---------------------------------------------------------------------------
template <int KC, bool MASS>
__global__ __launch_bounds__(256) void k_pa_cols(const PaWalk a) {
    const PaGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const int slot = t.slot();   // of a segment without rows too: its sums are zeros
    double bi[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) bi[c] = a.B[(size_t)(a.c0 + c) * g.m + t.ic];
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        double xr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) xr[jj] = a.x[walk_place(t, g, j0, jj)];
        bool keep[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) keep[jj] = t.in_i && j0 + jj < g.n && walk_keep(xr[jj], a.tol);
        int col;
        const bool owner = walk_col_owner(t, g, j0, col);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            double xv[TC];
#pragma unroll
            for (int jj = 0; jj < TC; ++jj) {
                const double xb = xr[jj] * bi[c];
                xv[jj] = keep[jj] ? xb : 0.0;
            }
            const double cs = colsum16(xv, t.lane);
            if (owner) a.part[pa_part_index(g, slot, c, col)] = cs;
        }
        if (MASS) {
            double xv[TC];
#pragma unroll
            for (int jj = 0; jj < TC; ++jj) xv[jj] = keep[jj] ? xr[jj] : 0.0;
            const double cs = colsum16(xv, t.lane);
            if (owner) a.part[pa_part_index(g, slot, PA_KC, col)] = cs;
        }
    }
}

// ---------------------------------------------------------------------------
// finishing kernel of a pass
// ---------------------------------------------------------------------------
struct PaFin {
    PaGeo g;
    int c0, kc;
    int first;         // pass 0: the mass comes out of the partials (and goes to w), later passes read w
    int normalize;
    const double* part;
    double* Y;
    double* w;         // R entries; nullptr: no mass wanted (then normalize is 0)
};

__global__ __launch_bounds__(256) void k_pa_fin(const PaFin a) {
    const PaGeo& g = a.g;
    const int R = pa_out_rows(g), S = pa_part_count(g);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)R * a.kc) return;
    const int c = (int)(t / R), r = (int)(t - (long long)c * R);
    double y = sum_strided(a.part + pa_part_index(g, 0, c, r), S, pa_part_stride(g));
    if (a.w) {
        double mass;
        if (a.first) {
            // every component's thread adds the same partials in the same order: the same bits
            mass = sum_strided(a.part + pa_part_index(g, 0, PA_KC, r), S, pa_part_stride(g));
            if (c == 0) a.w[r] = mass;
        } else {
            mass = a.w[r];
        }
        if (a.normalize) y = y / mass;
    }
    a.Y[(size_t)(a.c0 + c) * R + r] = y;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int KC, bool MASS>
void launch_walk(ipd_ctx* ctx, const PaWalk& a) {
    const dim3 grid(a.g.nib, a.g.ng);
    if (a.g.own.side == 0)
        hipLaunchKernelGGL((k_pa_rows<KC, MASS>), grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((k_pa_cols<KC, MASS>), grid, dim3(256), 0, ctx->stream, a);
    IPD_KERNEL_CHECK();
}

template <bool MASS>
void launch_walk_kc(ipd_ctx* ctx, int kc, const PaWalk& a) {
    switch (kc) {
        case 1: return launch_walk<1, MASS>(ctx, a);
        case 2: return launch_walk<2, MASS>(ctx, a);
        case 3: return launch_walk<3, MASS>(ctx, a);
        default: return launch_walk<PA_KC, MASS>(ctx, a);
    }
}
static_assert(PA_KC == 4, "launch_walk_kc instantiates KC = 1 .. 4");

void check_args(const ipd_apd* h, double tol, int32_t side, int32_t k, int32_t normalize, const double* B,
                const double* Y) {
    IPD_REQUIRE(h && B && Y, IPD_E_ARG, "ipd_apd_plan_apply: NULL argument");
    IPD_REQUIRE(side == 0 || side == 1, IPD_E_ARG, "ipd_apd_plan_apply: side must be 0 or 1");
    IPD_REQUIRE(normalize == 0 || normalize == 1, IPD_E_ARG, "ipd_apd_plan_apply: normalize must be 0 or 1");
    IPD_REQUIRE(tol >= 0.0, IPD_E_ARG, "ipd_apd_plan_apply: tol must be >= 0");   // false for a NaN
    IPD_REQUIRE(k >= 1 && k <= PA_KMAX, IPD_E_LIMIT, "ipd_apd_plan_apply: k must be in [1, 16]");
}

// all launches of a call on the context's stream; the caller waits for it
void plan_apply_dev(ipd_apd* h, double tol, int side, int k, int normalize, const double* B_dev, double* Y_dev,
                    double* w_dev) {
    ipd_ctx* ctx = h->ctx;
    Arena& S = *ctx->scratch;
    const PaGeo g = pa_make_geo(h->m, h->n, k, side);
    const int R = pa_out_rows(g);
    double* part = S.alloc<double>(pa_part_len(g));
    if (normalize && !w_dev) w_dev = S.alloc<double>((size_t)R);
    for (int p = 0; p < g.npass; ++p) {
        const int kc = pa_pass_kc(g, p);
        PaWalk a;
        a.g = g;
        a.c0 = pa_pass_c0(p);
        a.x = h->u;   // class 2: the x block of uk comes first
        a.B = B_dev;
        a.tol = tol;
        a.part = part;
        if (p == 0 && w_dev) launch_walk_kc<true>(ctx, kc, a);
        else launch_walk_kc<false>(ctx, kc, a);
        PaFin f;
        f.g = g;
        f.c0 = a.c0;
        f.kc = kc;
        f.first = p == 0;
        f.normalize = normalize;
        f.part = part;
        f.Y = Y_dev;
        f.w = w_dev;
        hipLaunchKernelGGL(k_pa_fin, dim3(cdiv((long long)R * kc, 256)), dim3(256), 0, ctx->stream, f);
        IPD_KERNEL_CHECK();
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_plan_apply_dev(ipd_apd* h, double tol, int32_t side, int32_t k, int32_t normalize,
                                      const double* B_dev, double* Y_dev, double* w_dev) {
    return ipd_guard([&] {
        check_args(h, tol, side, k, normalize, B_dev, Y_dev);
        CallScope scope(h->ctx);
        plan_apply_dev(h, tol, side, k, normalize, B_dev, Y_dev, w_dev);
        h->ctx->sync();   // the scratch arrays are the next call's
    });
}

extern "C" int ipd_apd_plan_apply(ipd_apd* h, double tol, int32_t side, int32_t k, int32_t normalize,
                                  const double* B, double* Y, double* w) {
    return ipd_guard([&] {
        check_args(h, tol, side, k, normalize, B, Y);
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        Arena& S = *ctx->scratch;
        const size_t rin = side ? (size_t)h->m : (size_t)h->n, rout = side ? (size_t)h->n : (size_t)h->m;
        double* B_dev = S.alloc<double>(rin * k);
        double* Y_dev = S.alloc<double>(rout * k);
        double* w_dev = w ? S.alloc<double>(rout) : nullptr;
        ctx->upload(B_dev, B, rin * k);
        plan_apply_dev(h, tol, side, k, normalize, B_dev, Y_dev, w_dev);
        ctx->fetch(Y_dev, Y, rout * k);
        if (w) ctx->fetch(w_dev, w, rout);
        ctx->sync();
    });
}
