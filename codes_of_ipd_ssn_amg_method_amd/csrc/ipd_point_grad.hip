// The gradient of the transport cost in the point positions, where the plan lives (ipd_apd_point_grad,
// ipd_apd_point_grad_dev): G(i,k) = sum_j X_ij * dc(xs_i, ys_j)/dxs(i,k) (side 0) or
// G(j,k) = sum_i X_ij * dc/dys(j,k) (side 1), X being what ipd_apd_plan would return at the same tol, with the mass
// of the kept entries and the counts of kept entries and of kept entries at a kink of c.  The weight depends on the
// pair (i, j), so this is no product X*B: it is recomputed from the (m+n)*d coordinates per entry of x.  c is never
// read -- a stored, a matrix-free and a host-c workspace run the same code -- and nothing of the workspace is written:
// the partials live in the context's scratch arena.
//
//   walk    one streaming read of x per pass of PG_KC = 4 output components, in the frame of ipd_walk_dev.h: lanes
//           along i, a wave walks WK_CPG chunks of TC columns alone, 16 clamped loads of x in flight, no LDS tile and
//           no barrier inside the chunk loop.  The row coordinates are registers for d <= 3 (cost_src_row<D>) and sit
//           in LDS as [k][thread] for larger d; the column coordinates of a chunk are fetched by the lanes for
//           walk_lane_col and handed round with __shfl.  A pass of metric 2 or 4 folds all d coordinates of a pair
//           again (a, k*).  A dropped entry, a padding lane and a clamped column contribute +0.0 through a select.
//     side 0  PG_KC row accumulators and the mass stay in registers over the column group: sequential in ascending j
//             from +0.0, one partial per (group, component, row).
//     side 1  per chunk and component one colsum16 butterfly, one partial per (segment slot, component, column).
//   finish  one thread per entry of the pass's components of G adds its partials in index order; pass 0 also sums the
//           mass into w and, in its first workgroup, the workgroups' integer counts into the statistics.
//
// One weight and every index: ipd_point_grad_geo.h.  Deterministic: every sum has a fixed shape that depends neither on
// d nor on the pass split, no float atomics -- two calls give the same bits, and so do the host and the device entry.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>
#include <vector>

#include "ipd_apd_state.h"
#include "ipd_point_grad_geo.h"
#include "ipd_walk_dev.h"

namespace {

// TR, TC: ipd_apd_geo.h; colsum16, sum_strided: ipd_apd_tiles.h
static_assert(PG_KC * TC == 64, "the lanes of a wave fetch a chunk's TC x PG_KC block of column coordinates in one load each");
static_assert(TR == 256 && APD_WAVES == 4, "the LDS form keeps [k][thread] for 256 threads");

struct PgWalk {
    PgGeo g;
    int c0, kc;        // first component of the pass, and how many
    int first;         // pass 0: the counts, and the mass when `mass`
    int mass;
    CostSrc src;       // coordinates, dimension, divider
    const double* x;
    double tol;
    double* part;      // pg_part_index; behind its pg_part_len entries the workgroups' counts, written by pass 0:
                       // [walk_block_index][PG_REC] 64-bit integers (one pointer less to hold over the walk)
};

// f(k) for the coordinates of a point (side 1: for the components of the pass): unrolled where D is a template
// parameter, so that no register array is indexed by a run-time k
template <int D, class F>
__device__ __forceinline__ void pg_each_k(int d, F&& f) {
    if constexpr (D > 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) f(k);
    } else {
#pragma nounroll
        for (int k = 0; k < d; ++k) f(k);
    }
}

// The value as it is, in a vector register, and nothing known about it: no instruction.  The kept entries of a chunk and
// the pairs' flags are bits of one vector register, since 16 lane masks held over a chunk take 32 scalar registers and
// spill; behind this the compiler tests a bit where it is used and does not collect the 16 tests as masks again.
template <class T>
__device__ __forceinline__ void pg_opaque(T& v) {
    asm volatile("" : "+v"(v));
}
// the same for a wave-uniform value in a scalar register: what is derived from it is derived where it is used
__device__ __forceinline__ void pg_opaque_uniform(int& v) {
    asm volatile("" : "+s"(v));
}

// D = 1 .. PG_DT_MAX: the row coordinates in registers, all D components in one pass.  D = 0: any d, the row coordinates
// in LDS, PG_KC components per pass (a short last pass computes a clamped coordinate again and leaves it unstored).
template <int D, int METRIC, int SIDE>
__global__ __launch_bounds__(256) void k_pg_walk(const PgWalk a) {
    constexpr bool REG = D > 0;
    constexpr int KC = REG ? D : PG_KC;
    __shared__ double xl[REG ? 1 : IPD_COST_DIM_MAX * 256];   // [k][thread]
    __shared__ int red[APD_WAVES * PG_REC];
    const PgGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);
    const int d = REG ? D : g.own.d;
    double xreg[REG ? D : 1];
    if constexpr (REG) {
        cost_src_row<KC>(a.src, t.ic, xreg);
    } else {
        // a thread reads back what it wrote itself: no barrier needed
        for (int k = 0; k < d; ++k) xl[k * 256 + t.tid] = a.src.xs[(size_t)k * g.m + t.ic];
    }
    auto xrow = [&](int k) -> double { return REG ? xreg[REG ? k : 0] : xl[k * 256 + t.tid]; };
    // metric 3 folds for its kink count only
    const bool fold = pg_needs_fold(METRIC) || (METRIC == COST_CITYBLOCK && a.first);
    const int slot = t.slot();
    int blk = walk_block_index(g, t.ib, t.grp);   // for the counts after the walk: in a vector register over it
    pg_opaque(blk);
    double acc[KC], wacc = 0.0;
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[c] = 0.0;
    int kept = 0, kinks = 0;
#pragma nounroll
    for (int ch = 0; ch < WK_CPG; ++ch) {
        const int j0 = walk_chunk_col(t.grp, ch);
        if (j0 >= g.n) break;  // uniform
        // the pass's numbers, per chunk: the components' offsets and tests are a few scalar operations, hoisted out
        // of the walk they would hold scalar registers over it
        int c0 = a.c0, kc = a.kc;
        if (!REG) {
            pg_opaque_uniform(c0);
            pg_opaque_uniform(kc);
        }
        double xr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) xr[jj] = a.x[walk_place(t, g, j0, jj)];
        const int jl = walk_lane_col(t, g, j0);
        PgPair f[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) f[jj] = pg_pair_init();
        unsigned flags = 0;
        if (fold) {
            pg_each_k<D>(d, [&](int k) {   // ascending k for every pair
                const double xk = xrow(k);
                const double yl = a.src.ys[(size_t)k * g.n + jl];
#pragma unroll
                for (int jj = 0; jj < TC; ++jj) pg_pair_fold<METRIC>(f[jj], flags, jj, k, xk, __shfl(yl, jj));
            });
#pragma unroll
            for (int jj = 0; jj < TC; ++jj) pg_pair_finish<METRIC>(f[jj]);
        }
        // the kept entries of the chunk as bits of a vector register: 16 lane masks would hold the scalar registers
        // the kernels cannot spare
        unsigned km = 0;
#pragma unroll
        for (int jj = 0; jj < TC; ++jj)
            km |= t.in_i && j0 + jj < g.n && walk_keep(xr[jj], a.tol) ? 1u << jj : 0u;
        if (a.first) {
            unsigned kk = 0;
#pragma unroll
            for (int jj = 0; jj < TC; ++jj) kk |= pg_pair_kink<METRIC>(f[jj], flags, jj) ? 1u << jj : 0u;
            kept += __popc(km);
            kinks += __popc(km & kk);
        }
        // lane l fetches coordinate (l >> 4) of the pass of column j0 + (l & 15), clamped to the last coordinate
        const int lc = t.lane >> 4;
        const int kl = REG ? min(lc, KC - 1) : min(c0 + lc, d - 1);
        const double yl = a.src.ys[(size_t)kl * g.n + jl];
        // what entry (jj, c) adds: x*h_k resp. x*(-h_k) when it is kept, else +0.0
        auto term = [&](int jj, int c) -> double {
            const int k = REG ? c : min(c0 + c, d - 1);
            const double xk = REG ? xreg[REG ? c : 0] : xl[k * 256 + t.tid];
            const double y = __shfl(yl, c * TC + jj);
            const double h = pg_scaled(pg_h<METRIC>(f[jj], k, xk, y), a.src.divide, a.src.denom);
            const double xh = pg_term(xr[jj], h, SIDE);
            return km >> jj & 1u ? xh : 0.0;
        };
        if (SIDE == 0) {
#pragma unroll
            for (int jj = 0; jj < TC; ++jj) {
                pg_opaque(km);   // (tested column by column, not held as 16 lane masks)
#pragma unroll
                for (int c = 0; c < KC; ++c) acc[c] += term(jj, c);   // (a short last pass: the clamped coordinate again)
                if (a.mass) wacc += km >> jj & 1u ? xr[jj] : 0.0;
            }
        } else {
            int col;
            const bool owner = walk_col_owner(t, g, j0, col);
            // (the LDS form: a loop over the pass's components that stays one, so that one component's offsets and
            // tests are live at a time)
            pg_each_k<D>(kc, [&](int c) {
                // every component tests the chunk's bits and the pairs' folds again: held over the components as lane
                // masks they would spill scalar registers
                pg_opaque(km);
#pragma unroll
                for (int jj = 0; jj < TC; ++jj) {
                    if (METRIC == COST_EUCLIDEAN) pg_opaque(f[jj].acc);
                    if (METRIC == COST_CHEBYSHEV) pg_opaque(f[jj].kstar);
                }
                double xv[TC];
#pragma unroll
                for (int jj = 0; jj < TC; ++jj) xv[jj] = term(jj, c);
                const double cs = colsum16(xv, t.lane);
                if (owner) a.part[pg_part_index(g, slot, c, col)] = cs;
            });
            if (a.mass) {
                double xv[TC];
#pragma unroll
                for (int jj = 0; jj < TC; ++jj) xv[jj] = km >> jj & 1u ? xr[jj] : 0.0;
                const double cs = colsum16(xv, t.lane);
                if (owner) a.part[pg_part_index(g, slot, PG_KC, col)] = cs;
            }
        }
    }
    if (SIDE == 0 && t.in_i) {
#pragma unroll
        for (int c = 0; c < KC; ++c)
            if (REG || c < a.kc) a.part[pg_part_index(g, t.grp, c, t.i)] = acc[c];
        if (a.mass) a.part[pg_part_index(g, t.grp, PG_KC, t.i)] = wacc;
    }
    if (a.first) {   // uniform: the workgroup's integer counts
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            kept += __shfl_xor(kept, s);
            kinks += __shfl_xor(kinks, s);
        }
        if (t.lane == 0) {
            red[t.wv * PG_REC] = kept;
            red[t.wv * PG_REC + 1] = kinks;
        }
        __syncthreads();
        if (t.tid < PG_REC) {
            long long r = 0;
#pragma unroll
            for (int w = 0; w < APD_WAVES; ++w) r += red[w * PG_REC + t.tid];
            long long* rec = reinterpret_cast<long long*>(a.part + pg_part_len(g));
            rec[(size_t)blk * PG_REC + t.tid] = r;
        }
    }
}

// ---------------------------------------------------------------------------
// finishing kernel of a pass
// ---------------------------------------------------------------------------
struct PgStatsDev {   // ipd_grad_stats
    long long kept, kinks;
    double denom;
};
static_assert(sizeof(PgStatsDev) == sizeof(ipd_grad_stats) && sizeof(PgStatsDev) == PG_STATS_DOUBLES * sizeof(double),
              "the device copy of the statistics");

struct PgFin {
    PgGeo g;
    int c0, kc;
    int first;         // pass 0: the mass (when w is given) and the counts
    double denom;      // what the statistics report: 1.0 without scale
    const double* part;   // and the counts behind it
    double* G;
    double* w;         // R entries or nullptr
    PgStatsDev* st;
};

__global__ __launch_bounds__(256) void k_pg_fin(const PgFin a) {
    __shared__ long long red[APD_WAVES * PG_REC];
    const PgGeo& g = a.g;
    const int R = pg_out_rows(g), S = pg_part_count(g);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < (long long)R * a.kc) {
        const int c = (int)(t / R), r = (int)(t - (long long)c * R);
        a.G[(size_t)(a.c0 + c) * R + r] = sum_strided(a.part + pg_part_index(g, 0, c, r), S, pg_part_stride(g));
        if (a.first && a.w && c == 0)
            a.w[r] = sum_strided(a.part + pg_part_index(g, 0, PG_KC, r), S, pg_part_stride(g));
    }
    if (a.first && blockIdx.x == 0) {   // uniform over the workgroup
        const int nblk = walk_blocks(g), tid = threadIdx.x;
        const long long* rec = reinterpret_cast<const long long*>(a.part + pg_part_len(g));
        long long kept = 0, kinks = 0;
        for (int b = tid; b < nblk; b += 256) {
            kept += rec[(size_t)b * PG_REC];
            kinks += rec[(size_t)b * PG_REC + 1];
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            kept += __shfl_xor(kept, s);
            kinks += __shfl_xor(kinks, s);
        }
        if ((tid & 63) == 0) {
            red[(tid >> 6) * PG_REC] = kept;
            red[(tid >> 6) * PG_REC + 1] = kinks;
        }
        __syncthreads();
        if (tid == 0) {
            long long k0 = 0, k1 = 0;
#pragma unroll
            for (int w = 0; w < APD_WAVES; ++w) {
                k0 += red[w * PG_REC];
                k1 += red[w * PG_REC + 1];
            }
            a.st->kept = k0;
            a.st->kinks = k1;
            a.st->denom = a.denom;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int D, int METRIC>
void launch_walk_side(ipd_ctx* ctx, const PgWalk& a) {
    const dim3 grid(a.g.nib, a.g.ng);
    if (a.g.own.side == 0)
        hipLaunchKernelGGL((k_pg_walk<D, METRIC, 0>), grid, dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((k_pg_walk<D, METRIC, 1>), grid, dim3(256), 0, ctx->stream, a);
    IPD_KERNEL_CHECK();
}

template <int METRIC>
void launch_walk_dim(ipd_ctx* ctx, const PgWalk& a) {
    switch (a.src.dim > PG_DT_MAX ? 0 : a.src.dim) {
        case 1: return launch_walk_side<1, METRIC>(ctx, a);
        case 2: return launch_walk_side<2, METRIC>(ctx, a);
        case 3: return launch_walk_side<3, METRIC>(ctx, a);
        default: return launch_walk_side<0, METRIC>(ctx, a);
    }
}
static_assert(PG_DT_MAX == 3, "launch_walk_dim instantiates D = 1, 2, 3");

void launch_walk(ipd_ctx* ctx, const PgWalk& a) {
    switch (a.src.metric) {
        case COST_SQEUCLIDEAN: return launch_walk_dim<COST_SQEUCLIDEAN>(ctx, a);
        case COST_EUCLIDEAN: return launch_walk_dim<COST_EUCLIDEAN>(ctx, a);
        case COST_CITYBLOCK: return launch_walk_dim<COST_CITYBLOCK>(ctx, a);
        case COST_CHEBYSHEV: return launch_walk_dim<COST_CHEBYSHEV>(ctx, a);
        default: throw IpdError(IPD_E_ARG, COST_CHECK_TEXT[COST_METRIC]);
    }
}

void check_args(const ipd_apd* h, double tol, int32_t side, const double* G) {
    IPD_REQUIRE(h && G, IPD_E_ARG, "ipd_apd_point_grad: NULL argument");
    IPD_REQUIRE(side == 0 || side == 1, IPD_E_ARG, "ipd_apd_point_grad: side must be 0 or 1");
    IPD_REQUIRE(tol >= 0.0, IPD_E_ARG, "ipd_apd_point_grad: tol must be >= 0");   // false for a NaN
}

// the workspace's own coordinates and divider
CostSrc own_source(const ipd_apd* h) {
    IPD_REQUIRE(h->cost_src.xs && h->cost_src.ys, IPD_E_ARG,
                "ipd_apd_point_grad: the workspace was made from a host c and has no points; give a specification");
    return h->cost_src;
}

// a given specification on device coordinates; scale = 1: the divider comes from the build's reduction without a
// destination (one read-back of its own, the stream is waited for)
CostSrc given_source(ipd_apd* h, int metric, int dim, int scale, const double* xs_dev, const double* ys_dev) {
    CostSrc s{};
    s.xs = xs_dev;
    s.ys = ys_dev;
    s.m = h->m;
    s.n = h->n;
    s.dim = dim;
    s.metric = metric;
    s.divide = scale;
    s.denom = scale ? apd_cost_largest(h->ctx, metric, dim, h->m, h->n, xs_dev, ys_dev) : 0.0;
    return s;
}

// all launches of a call on the context's stream; the caller reads *st_dev back and so waits for it
void point_grad_dev(ipd_apd* h, const CostSrc& src, double tol, int side, double* G_dev, double* w_dev,
                    PgStatsDev* st_dev) {
    ipd_ctx* ctx = h->ctx;
    Arena& S = *ctx->scratch;
    const PgGeo g = pg_make_geo(h->m, h->n, src.dim, side);
    static_assert(sizeof(long long) == sizeof(double), "the counts lie behind the partials");
    double* part = S.alloc<double>(pg_part_len(g) + pg_rec_len(g));
    for (int p = 0; p < g.npass; ++p) {
        PgWalk a;
        a.g = g;
        a.c0 = pg_pass_c0(p);
        a.kc = pg_pass_kc(g, p);
        a.first = p == 0;
        a.mass = p == 0 && w_dev;
        a.src = src;
        a.x = h->u;   // class 2: the x block of uk comes first
        a.tol = tol;
        a.part = part;
        launch_walk(ctx, a);
        PgFin f;
        f.g = g;
        f.c0 = a.c0;
        f.kc = a.kc;
        f.first = a.first;
        f.denom = src.divide ? src.denom : 1.0;
        f.part = part;
        f.G = G_dev;
        f.w = w_dev;
        f.st = st_dev;
        hipLaunchKernelGGL(k_pg_fin, dim3(cdiv((long long)pg_out_rows(g) * a.kc, 256)), dim3(256), 0, ctx->stream, f);
        IPD_KERNEL_CHECK();
    }
}

void store_stats(const PgStatsDev& s, ipd_grad_stats* st) {
    if (!st) return;
    st->kept = s.kept;
    st->kinks = s.kinks;
    st->denom = s.denom;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_point_grad_dev(ipd_apd* h, int32_t metric, int32_t dim, int32_t scale, const double* xs_dev,
                                      const double* ys_dev, double tol, int32_t side, double* G_dev, double* w_dev,
                                      ipd_grad_stats* st) {
    return ipd_guard([&] {
        check_args(h, tol, side, G_dev);
        IPD_REQUIRE(!xs_dev == !ys_dev, IPD_E_ARG, "ipd_apd_point_grad_dev: exactly one of xs_dev, ys_dev is NULL");
        if (xs_dev) {
            IPD_REQUIRE(metric >= COST_SQEUCLIDEAN && metric <= COST_CHEBYSHEV, IPD_E_ARG, COST_CHECK_TEXT[COST_METRIC]);
            IPD_REQUIRE(dim >= 1 && dim <= IPD_COST_DIM_MAX, IPD_E_ARG, COST_CHECK_TEXT[COST_DIM]);
            IPD_REQUIRE(scale == 0 || scale == 1, IPD_E_ARG, COST_CHECK_TEXT[COST_SCALE]);
        }
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        const CostSrc src = xs_dev ? given_source(h, metric, dim, scale, xs_dev, ys_dev) : own_source(h);
        PgStatsDev* st_dev = reinterpret_cast<PgStatsDev*>(ctx->scratch->alloc<double>(PG_STATS_DOUBLES));
        point_grad_dev(h, src, tol, side, G_dev, w_dev, st_dev);
        PgStatsDev got;
        ctx->fetch_bytes(st_dev, &got, sizeof(got));   // waits for the stream: the scratch arrays are the next call's
        store_stats(got, st);
    });
}

extern "C" int ipd_apd_point_grad(ipd_apd* h, const ipd_cost_spec* s, double tol, int32_t side, double* G, double* w,
                                  ipd_grad_stats* st) {
    return ipd_guard([&] {
        check_args(h, tol, side, G);
        if (s) {
            const CostCheck ck = cost_spec_check(s->metric, s->dim, s->m, s->n, s->xs, s->ys, s->scale);
            IPD_REQUIRE(ck == COST_OK, ck == COST_SHAPE ? IPD_E_LIMIT : IPD_E_ARG, COST_CHECK_TEXT[ck]);
            IPD_REQUIRE(s->m == h->m && s->n == h->n, IPD_E_ARG,
                        "ipd_apd_point_grad: m, n of the spec and of the workspace differ");
        }
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        Arena& S = *ctx->scratch;
        CostSrc src;
        if (s) {
            const size_t m = (size_t)h->m, n = (size_t)h->n, dim = (size_t)s->dim;
            double* xs_dev = S.alloc<double>(m * dim);
            double* ys_dev = S.alloc<double>(n * dim);
            ctx->upload(xs_dev, s->xs, m * dim);
            ctx->upload(ys_dev, s->ys, n * dim);
            src = given_source(h, s->metric, s->dim, s->scale, xs_dev, ys_dev);
        } else {
            src = own_source(h);
        }
        // one block [statistics; G; w], one read-back
        const size_t R = side ? (size_t)h->n : (size_t)h->m, cnt = (size_t)PG_STATS_DOUBLES + R * src.dim + (w ? R : 0);
        double* out_dev = S.alloc<double>(cnt);
        double* G_dev = out_dev + PG_STATS_DOUBLES;
        double* w_dev = w ? G_dev + R * src.dim : nullptr;
        point_grad_dev(h, src, tol, side, G_dev, w_dev, reinterpret_cast<PgStatsDev*>(out_dev));
        std::vector<double> out(cnt);
        ctx->fetch(out_dev, out.data(), cnt);   // waits for the stream
        PgStatsDev got;
        std::memcpy(&got, out.data(), sizeof(got));
        std::memcpy(G, out.data() + PG_STATS_DOUBLES, R * src.dim * sizeof(double));
        if (w) std::memcpy(w, out.data() + PG_STATS_DOUBLES + R * src.dim, R * sizeof(double));
        store_stats(got, st);
    });
}
