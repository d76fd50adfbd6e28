// The cost matrix built on the device from two point clouds (ipd_cost_points_dev, ipd_apd_create_points,
// ipd_apd_get_cost).
//
// c(i,j) = metric(xs(i,:), ys(j,:)) is a function of (m+n)*d numbers; only those cross the host boundary, the mn
// entries are made where the drivers read them.  Coordinates are coordinate-major (xs[i + k*m], ys[j + k*n]), the
// result column-major (c[i + j*m]) as everywhere in the drivers.
//
//   build   the walk of the plan kernels (ipd_plan.hip; the geometry is ipd_cost_plan.h's): lanes along i, a wave
//           owns 64 (or, with two rows per lane, 128) consecutive rows and walks 16*reps columns alone.  The row
//           coordinates are registers for d <= 3 (one instantiation per d) and come out of LDS, filled once before
//           the walk, for larger d; the column coordinates are wave-uniform loads.  No barrier in the column loop,
//           one store instruction per column and wave (512 or 1024 contiguous bytes).  Minimum, maximum and sum
//           of what is stored leave as per-workgroup partials in the same pass.
//   scale   the build kernel runs twice: first without a store (the partials give the largest entry, which the
//           host has to see anyway: 0 or inf is an error), then it recomputes, divides and stores.  One write of
//           8*mn bytes, no read-back.
//   finish  one workgroup adds the partials in workgroup order and a fixed tree (as k_plan_fin): no float
//           atomics, two calls give the same bits.
//   free    ipd_apd_create_points_free keeps the coordinates in the workspace and stores no
//           c: the build kernel runs without a store, for the largest entry (scale) and for the statistics of what
//           a stored workspace would hold, and ipd_apd_get_cost builds the matrix into scratch memory on demand.
//           The passes that read c(i,j) recompute it (CostFree<D>, ipd_apd_tiles.h).
//
// An entry is folded by cost_fold / cost_finish of ipd_cost_plan.h, the code its CPU test runs.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdint>

#include "ipd_apd_state.h"
#include "ipd_cost_plan.h"

namespace {

constexpr int CSC = 3;   // statistics per workgroup: min, max, sum

struct CostArgs {
    CostGeo g;
    int d;
    double denom;       // divide != 0: every entry is divided by it
    int divide;
    double* part;       // [workgroup][CSC]
};
// The arrays are kernel parameters of their own, __restrict__: only then may the compiler fetch the wave-uniform
// column coordinates with scalar loads while the same kernel stores to c.
//   xs m*d, ys n*d; c mn, or nullptr: statistics only
#define COST_ARRAYS const double* __restrict__ xs, const double* __restrict__ ys, double* __restrict__ c

__device__ __forceinline__ double wave_add(double v) {   // butterfly: every lane ends with the same bits
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

struct CostAcc {
    double lo, hi, sum;
    __device__ __forceinline__ void take(double v) {
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        sum += v;
    }
};
__device__ __forceinline__ CostAcc cost_acc_init() {
    CostAcc s;
    s.lo = __builtin_inf();
    s.hi = -__builtin_inf();
    s.sum = 0.0;
    return s;
}

// the lanes' statistics -> the workgroup's partial: wave butterflies, then the four waves in order
__device__ __forceinline__ void cost_block_partial(const CostAcc& s, double* red, double* part, int blk) {
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const double w0 = wave_min(s.lo), w1 = wave_max(s.hi), w2 = wave_add(s.sum);
    if (lane == 0) {
        red[wv * CSC + 0] = w0;
        red[wv * CSC + 1] = w1;
        red[wv * CSC + 2] = w2;
    }
    __syncthreads();
    if (tid < CSC) {
        const double r0 = red[tid], r1 = red[CSC + tid], r2 = red[2 * CSC + tid], r3 = red[3 * CSC + tid];
        double r;
        if (tid == 0) {
            r = r1 < r0 ? r1 : r0;
            r = r2 < r ? r2 : r;
            r = r3 < r ? r3 : r;
        } else if (tid == 1) {
            r = r1 > r0 ? r1 : r0;
            r = r2 > r ? r2 : r;
            r = r3 > r ? r3 : r;
        } else {
            r = r0 + r1 + r2 + r3;
        }
        part[(size_t)blk * CSC + tid] = r;
    }
}

// ---------------------------------------------------------------------------
// build: D = 1..COST_DT_MAX, the row coordinates in registers; RPL rows per lane
// ---------------------------------------------------------------------------
template <int D, int RPL, int METRIC>
__global__ __launch_bounds__(256) void k_cost_build(const CostArgs a, COST_ARRAYS) {
    __shared__ double red[COST_WAVES * CSC];
    const CostGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ib = blockIdx.x, jg = blockIdx.y;
    const int i = cost_lane_row(g, ib, wv, lane);
    // RPL == 2 runs on an even m only: the lane's two rows are inside together
    const bool in_i = i < g.m;
    const int ic = in_i ? i : g.m - RPL;
    double xr[D][RPL];
#pragma unroll
    for (int k = 0; k < D; ++k)
#pragma unroll
        for (int r = 0; r < RPL; ++r) xr[k][r] = xs[(size_t)k * g.m + ic + r];
    CostAcc st = cost_acc_init();
    for (int rep = 0; rep < g.reps; ++rep) {
        const int j0 = cost_step_col(g, jg, rep);
        if (j0 >= g.n) break;  // uniform
#pragma unroll
        for (int jj = 0; jj < COST_TC; ++jj) {
            const int j = min(j0 + jj, g.n - 1);   // uniform; clamped: the loads need no branch
            double acc[RPL];
#pragma unroll
            for (int r = 0; r < RPL; ++r) acc[r] = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double y = ys[(size_t)k * g.n + j];
#pragma unroll
                for (int r = 0; r < RPL; ++r) acc[r] = cost_fold<METRIC>(acc[r], xr[k][r], y);
            }
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
                acc[r] = cost_finish<METRIC>(acc[r]);
                if (a.divide) acc[r] = acc[r] / a.denom;
            }
            if (in_i && j0 + jj < g.n) {
#pragma unroll
                for (int r = 0; r < RPL; ++r) st.take(acc[r]);
                if (c) {
                    double* const dst = c + (size_t)j * g.m + i;
                    if (RPL == 2) *reinterpret_cast<double2*>(dst) = make_double2(acc[0], acc[RPL - 1]);
                    else *dst = acc[0];
                }
            }
        }
    }
    cost_block_partial(st, red, a.part, jg * gridDim.x + ib);
}

// ---------------------------------------------------------------------------
// build, any d: the workgroup's row coordinates in LDS (one row per lane), k outside the 16 columns
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(256) void k_cost_build_any(const CostArgs a, COST_ARRAYS) {
    __shared__ double red[COST_WAVES * CSC];
    __shared__ double xl[IPD_COST_DIM_MAX * 256];   // [k][thread]
    const CostGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ib = blockIdx.x, jg = blockIdx.y;
    const int i = cost_lane_row(g, ib, wv, lane);
    const bool in_i = i < g.m;
    const int ic = in_i ? i : g.m - 1;
    // a thread reads back what it wrote itself: no barrier needed
    for (int k = 0; k < a.d; ++k) xl[k * 256 + tid] = xs[(size_t)k * g.m + ic];
    CostAcc st = cost_acc_init();
    for (int rep = 0; rep < g.reps; ++rep) {
        const int j0 = cost_step_col(g, jg, rep);
        if (j0 >= g.n) break;  // uniform
        double acc[COST_TC];
#pragma unroll
        for (int jj = 0; jj < COST_TC; ++jj) acc[jj] = 0.0;
        for (int k = 0; k < a.d; ++k) {   // ascending k for every entry
            const double x = xl[k * 256 + tid];
            // lane jj fetches the coordinate of column j0 + jj (16 uniform loads and their clamped offsets held
            // more scalar registers than there are, as in k_plan_count)
            const double yl = ys[(size_t)k * g.n + min(j0 + (lane & (COST_TC - 1)), g.n - 1)];
#pragma unroll
            for (int jj = 0; jj < COST_TC; ++jj) acc[jj] = cost_fold<METRIC>(acc[jj], x, __shfl(yl, jj));
        }
#pragma unroll
        for (int jj = 0; jj < COST_TC; ++jj) {
            double v = cost_finish<METRIC>(acc[jj]);
            if (a.divide) v = v / a.denom;
            if (in_i && j0 + jj < g.n) {
                st.take(v);
                if (c) c[(size_t)(j0 + jj) * g.m + i] = v;
            }
        }
    }
    cost_block_partial(st, red, a.part, jg * gridDim.x + ib);
}

// ---------------------------------------------------------------------------
// the statistics of a matrix that is already there (ipd_apd_get_cost on a workspace made from a host c)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cost_stats(const CostArgs a, const double* __restrict__ src) {
    __shared__ double red[COST_WAVES * CSC];
    const CostGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ib = blockIdx.x, jg = blockIdx.y;
    const int i = cost_lane_row(g, ib, wv, lane);
    const bool in_i = i < g.m;
    const int ic = in_i ? i : g.m - 1;
    CostAcc st = cost_acc_init();
    for (int rep = 0; rep < g.reps; ++rep) {
        const int j0 = cost_step_col(g, jg, rep);
        if (j0 >= g.n) break;  // uniform
        double v[COST_TC];
#pragma unroll
        for (int jj = 0; jj < COST_TC; ++jj) v[jj] = src[(size_t)min(j0 + jj, g.n - 1) * g.m + ic];
#pragma unroll
        for (int jj = 0; jj < COST_TC; ++jj)
            if (in_i && j0 + jj < g.n) st.take(v[jj]);
    }
    cost_block_partial(st, red, a.part, jg * gridDim.x + ib);
}

// ---------------------------------------------------------------------------
// finish: thread t takes workgroups t, t+256, ... in that order, then the 256 threads meet in a fixed tree
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cost_fin(int nblk, const double* __restrict__ part,
                                                  ipd_cost_stats* __restrict__ out) {
    __shared__ double red[COST_WAVES * CSC];
    CostAcc s = cost_acc_init();
    for (int b = threadIdx.x; b < nblk; b += 256) {
        const double lo = part[(size_t)b * CSC], hi = part[(size_t)b * CSC + 1], sum = part[(size_t)b * CSC + 2];
        s.lo = lo < s.lo ? lo : s.lo;
        s.hi = hi > s.hi ? hi : s.hi;
        s.sum += sum;
    }
    __shared__ double fin[CSC];
    cost_block_partial(s, red, fin, 0);
    __syncthreads();
    if (threadIdx.x == 0) {
        out->min = fin[0];
        out->max = fin[1];
        out->sum = fin[2];
    }
}

__global__ __launch_bounds__(256) void k_cost_ones(size_t count, double* __restrict__ v) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (size_t)gridDim.x * 256) v[t] = 1.0;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int METRIC>
void launch_build_metric(ipd_ctx* ctx, const CostArgs& a, const double* xs, const double* ys, double* c) {
    const dim3 grid(a.g.nib, a.g.njg), block(256);
    const int key = a.d > COST_DT_MAX ? 0 : a.d * 2 + (a.g.rpl - 1);
    switch (key) {
        case 0: hipLaunchKernelGGL((k_cost_build_any<METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        case 2: hipLaunchKernelGGL((k_cost_build<1, 1, METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        case 3: hipLaunchKernelGGL((k_cost_build<1, 2, METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        case 4: hipLaunchKernelGGL((k_cost_build<2, 1, METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        case 5: hipLaunchKernelGGL((k_cost_build<2, 2, METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        case 6: hipLaunchKernelGGL((k_cost_build<3, 1, METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        case 7: hipLaunchKernelGGL((k_cost_build<3, 2, METRIC>), grid, block, 0, ctx->stream, a, xs, ys, c); break;
        default: throw IpdError(IPD_E_ARG, "cost build: no kernel for this dimension");
    }
    IPD_KERNEL_CHECK();
}
static_assert(COST_DT_MAX == 3, "launch_build_metric instantiates d = 1, 2, 3");

void launch_build(ipd_ctx* ctx, int metric, const CostArgs& a, const double* xs, const double* ys, double* c) {
    switch (metric) {
        case COST_SQEUCLIDEAN: launch_build_metric<COST_SQEUCLIDEAN>(ctx, a, xs, ys, c); break;
        case COST_EUCLIDEAN: launch_build_metric<COST_EUCLIDEAN>(ctx, a, xs, ys, c); break;
        case COST_CITYBLOCK: launch_build_metric<COST_CITYBLOCK>(ctx, a, xs, ys, c); break;
        case COST_CHEBYSHEV: launch_build_metric<COST_CHEBYSHEV>(ctx, a, xs, ys, c); break;
        default: throw IpdError(IPD_E_ARG, COST_CHECK_TEXT[COST_METRIC]);
    }
}

// the partials of the launch before -> *st (the stream is waited for)
void finish_stats(ipd_ctx* ctx, const CostArgs& a, ipd_cost_stats* dst, ipd_cost_stats* st) {
    hipLaunchKernelGGL(k_cost_fin, dim3(1), dim3(256), 0, ctx->stream, a.g.nib * a.g.njg, a.part, dst);
    IPD_KERNEL_CHECK();
    ctx->fetch_bytes(dst, st, sizeof(ipd_cost_stats));
}

// scale = 1: the largest entry of the unscaled cost, from the build without a destination in the geometry of `a` (whose
// partials and *dst it uses); *st receives that pass's statistics.  IPD_E_ARG when it is 0 or not finite.
double cost_largest(ipd_ctx* ctx, int metric, const CostArgs& a, const double* xs_dev, const double* ys_dev,
                    ipd_cost_stats* dst, ipd_cost_stats* st) {
    launch_build(ctx, metric, a, xs_dev, ys_dev, nullptr);
    finish_stats(ctx, a, dst, st);
    IPD_REQUIRE(cost_scale_ok(st->max), IPD_E_ARG, "cost spec: scale = 1 and the largest entry is 0 or not finite");
    return st->max;
}

void check_spec(const ipd_cost_spec* s) {
    const CostCheck ck = cost_spec_check(s->metric, s->dim, s->m, s->n, s->xs, s->ys, s->scale);
    IPD_REQUIRE(ck == COST_OK, ck == COST_SHAPE ? IPD_E_LIMIT : IPD_E_ARG, COST_CHECK_TEXT[ck]);
}

// The coordinates on the device -> c_dev (mn) and the statistics of what is stored; c_dev == nullptr stores
// nothing and gives the statistics of what would be stored.  `aligned16` is the alignment of the array that is, or
// would be, stored to: it decides the rows per lane, and with them the order in which the sum is added.  *src (or
// nullptr) receives the source the matrix-free passes recompute an entry from.  The stream has been waited for
// when this returns.
void cost_build_dev(ipd_ctx* ctx, const ipd_cost_spec* s, const double* xs_dev, const double* ys_dev, double* c_dev,
                    bool aligned16, ipd_cost_stats* st, CostSrc* src) {
    Arena& S = *ctx->scratch;
    const int m = (int)s->m, n = (int)s->n, d = s->dim;
    CostArgs a{};
    a.g = cost_geo(m, n, cost_rows_per_lane(m, d, aligned16, switch_value("IPD_COST_STORE")));
    a.d = d;
    a.part = S.alloc<double>((size_t)a.g.nib * a.g.njg * CSC);
    ipd_cost_stats* dst = reinterpret_cast<ipd_cost_stats*>(S.alloc<double>(sizeof(ipd_cost_stats) / sizeof(double)));
    if (s->scale) {
        a.denom = cost_largest(ctx, s->metric, a, xs_dev, ys_dev, dst, st);
        a.divide = 1;
    }
    launch_build(ctx, s->metric, a, xs_dev, ys_dev, c_dev);
    finish_stats(ctx, a, dst, st);
    if (src) {
        src->xs = xs_dev;
        src->ys = ys_dev;
        src->m = m;
        src->n = n;
        src->dim = d;
        src->metric = s->metric;
        src->divide = a.divide;
        src->denom = a.denom;
    }
}

// A checked specification -> c_dev (mn) and the statistics of what is stored.  The caller holds a CallScope;
// the stream has been waited for when this returns (the scratch arrays are the next call's).
void cost_from_points(ipd_ctx* ctx, const ipd_cost_spec* s, double* c_dev, ipd_cost_stats* st,
                      CostSrc* src = nullptr) {
    Arena& S = *ctx->scratch;
    const int m = (int)s->m, n = (int)s->n, d = s->dim;
    double* xs_dev = S.alloc<double>((size_t)m * d);
    double* ys_dev = S.alloc<double>((size_t)n * d);
    ctx->upload(xs_dev, s->xs, (size_t)m * d);
    ctx->upload(ys_dev, s->ys, (size_t)n * d);
    cost_build_dev(ctx, s, xs_dev, ys_dev, c_dev, (reinterpret_cast<uintptr_t>(c_dev) & 15) == 0, st, src);
}

void fill_ones(ipd_ctx* ctx, size_t mn, double* phi_ones_dev) {
    hipLaunchKernelGGL(k_cost_ones, dim3(elems_grid((long long)mn)), dim3(256), 0, ctx->stream, mn, phi_ones_dev);
    IPD_KERNEL_CHECK();
}

void note_spec(ipd_apd* h, const ipd_cost_spec* s) {
    h->cost_dim = s->dim;
    h->cost_metric = s->metric;
    h->cost_scale = s->scale;
}

// A stored workspace made from points keeps what the matrix-free one keeps, the (m+n)*dim coordinates in its arena and
// the divider, for the calls that differentiate in the positions (ipd_point_grad.hip).  Its passes go on reading the
// stored c: cost_free stays false and ipd_apd_cost_info answers what it answered.  `built`: what cost_build_dev left,
// its coordinate pointers were the build's scratch.  The coordinates go up a second time, 8*(m+n)*dim bytes once per
// create: the build runs inside apd_create_common's fill callback, which has no workspace to allocate from yet.
void keep_points(ipd_ctx* ctx, ipd_apd* h, const ipd_cost_spec* s, const CostSrc& built) {
    CallScope scope(ctx);
    const size_t m = (size_t)s->m, n = (size_t)s->n, dim = (size_t)s->dim;
    double* xs_dev = h->arena->alloc<double>(m * dim);
    double* ys_dev = h->arena->alloc<double>(n * dim);
    ctx->upload(xs_dev, s->xs, m * dim);
    ctx->upload(ys_dev, s->ys, n * dim);   // (an upload has taken its bytes when it returns)
    h->cost_src = built;
    h->cost_src.xs = xs_dev;
    h->cost_src.ys = ys_dev;
}

}  // namespace

// The largest entry of the unscaled cost of device coordinates, the number by which k_cost_build divides under
// scale = 1: the build without a destination (any dim: beyond COST_DT_MAX a statistics-only pass of the generic form).
// A maximum does not depend on the order it is taken in, so the rows per lane do not matter.  IPD_E_ARG when it is 0 or
// not finite.  The caller holds a CallScope; the stream has been waited for when this returns.
double apd_cost_largest(ipd_ctx* ctx, int metric, int dim, int m, int n, const double* xs_dev, const double* ys_dev) {
    Arena& S = *ctx->scratch;
    CostArgs a{};
    a.g = cost_geo(m, n, 1);
    a.d = dim;
    a.part = S.alloc<double>((size_t)a.g.nib * a.g.njg * CSC);
    ipd_cost_stats* dst = reinterpret_cast<ipd_cost_stats*>(S.alloc<double>(sizeof(ipd_cost_stats) / sizeof(double)));
    ipd_cost_stats st;
    return cost_largest(ctx, metric, a, xs_dev, ys_dev, dst, &st);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_cost_points_dev(ipd_ctx* ctx, const ipd_cost_spec* s, double* c_dev, ipd_cost_stats* st) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && s && c_dev, IPD_E_ARG, "ipd_cost_points_dev: NULL argument");
        check_spec(s);
        CallScope scope(ctx);
        ipd_cost_stats local;
        cost_from_points(ctx, s, c_dev, st ? st : &local);
    });
}

extern "C" int ipd_apd_create_points(ipd_ctx* ctx, const ipd_apd_data* d, const ipd_cost_spec* s, ipd_apd** out) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && d && s && out, IPD_E_ARG, "ipd_apd_create_points: NULL argument");
        IPD_REQUIRE(!d->c, IPD_E_ARG, "ipd_apd_create_points: c must be NULL (the cost comes from the points)");
        check_spec(s);
        IPD_REQUIRE(s->m == d->m && s->n == d->n, IPD_E_ARG, "ipd_apd_create_points: m, n of the spec and of the data differ");
        CostSrc built{};
        const ApdCostFill fill = [&](double* c_dev, double* phi_ones_dev, ipd_cost_stats* st) {
            CallScope scope(ctx);
            if (phi_ones_dev) fill_ones(ctx, (size_t)s->m * (size_t)s->n, phi_ones_dev);
            cost_from_points(ctx, s, c_dev, st, &built);
        };
        ipd_apd* h = nullptr;
        apd_create_common(ctx, d, &fill, &h);
        note_spec(h, s);
        try {
            keep_points(ctx, h, s, built);
        } catch (...) {
            ipd_apd_destroy(h);
            throw;
        }
        *out = h;
    });
}

extern "C" int ipd_apd_create_points_free(ipd_ctx* ctx, const ipd_apd_data* d, const ipd_cost_spec* s,
                                          ipd_apd** out) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && d && s && out, IPD_E_ARG, "ipd_apd_create_points_free: NULL argument");
        IPD_REQUIRE(!d->c, IPD_E_ARG, "ipd_apd_create_points_free: c must be NULL (the cost comes from the points)");
        check_spec(s);
        IPD_REQUIRE(cost_free_check(s->dim) == COST_FREE_OK, IPD_E_LIMIT, COST_FREE_TEXT[COST_FREE_DIM]);
        IPD_REQUIRE(s->m == d->m && s->n == d->n, IPD_E_ARG,
                    "ipd_apd_create_points_free: m, n of the spec and of the data differ");
        const ApdCostFree free_fill = [&](ipd_apd* h, double* phi_ones_dev) {
            CallScope scope(ctx);
            const size_t m = (size_t)s->m, n = (size_t)s->n, dim = (size_t)s->dim;
            if (phi_ones_dev) fill_ones(ctx, m * n, phi_ones_dev);
            // the coordinates are the workspace's own: its passes read them for as long as it lives
            double* xs_dev = h->arena->alloc<double>(m * dim);
            double* ys_dev = h->arena->alloc<double>(n * dim);
            ctx->upload(xs_dev, s->xs, m * dim);
            ctx->upload(ys_dev, s->ys, n * dim);
            // the statistics of what a stored workspace would hold, in its geometry: the workspace's c comes out
            // of the arena, 16-byte aligned
            cost_build_dev(ctx, s, xs_dev, ys_dev, nullptr, true, &h->cost_stats, &h->cost_src);
            h->cost_free = true;
            note_spec(h, s);
        };
        apd_create_common(ctx, d, nullptr, out, &free_fill);
    });
}

extern "C" int ipd_apd_cost_info(ipd_apd* h, ipd_cost_info* info) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && info, IPD_E_ARG, "ipd_apd_cost_info: NULL argument");
        info->form = h->cost_free ? 1 : 0;
        info->dim = h->cost_dim;
        info->metric = h->cost_metric;
        info->scale = h->cost_scale;
        info->device_bytes = h->cost_free ? (int64_t)(8 * ((size_t)h->m + (size_t)h->n) * (size_t)h->cost_dim)
                                          : (int64_t)(8 * h->mn);
    });
}

extern "C" int ipd_apd_get_cost(ipd_apd* h, double* c, ipd_cost_stats* st) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "ipd_apd_get_cost: NULL handle");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        if (c && h->cost_free) {
            // matrix-free: the matrix exists for this call only, in the scratch arena (given back with the scope)
            double* c_dev = ctx->scratch->alloc<double>(h->mn);
            const CostSrc& src = h->cost_src;
            CostArgs a{};
            a.g = cost_geo(h->m, h->n, cost_rows_per_lane(h->m, src.dim, (reinterpret_cast<uintptr_t>(c_dev) & 15) == 0,
                                                          switch_value("IPD_COST_STORE")));
            a.d = src.dim;
            a.denom = src.denom;
            a.divide = src.divide;
            a.part = ctx->scratch->alloc<double>((size_t)a.g.nib * a.g.njg * CSC);
            launch_build(ctx, src.metric, a, src.xs, src.ys, c_dev);
            ctx->fetch(c_dev, c, h->mn);
        } else if (c) {
            ctx->fetch(h->c, c, h->mn);
        }
        if (!st) return;
        if (!h->have_cost_stats) {
            Arena& S = *ctx->scratch;
            CostArgs a{};
            a.g = cost_geo(h->m, h->n, 1);
            a.part = S.alloc<double>((size_t)a.g.nib * a.g.njg * CSC);
            ipd_cost_stats* dst =
                reinterpret_cast<ipd_cost_stats*>(S.alloc<double>(sizeof(ipd_cost_stats) / sizeof(double)));
            hipLaunchKernelGGL(k_cost_stats, dim3(a.g.nib, a.g.njg), dim3(256), 0, ctx->stream, a,
                               (const double*)h->c);
            IPD_KERNEL_CHECK();
            finish_stats(ctx, a, dst, &h->cost_stats);
            h->have_cost_stats = true;
        }
        *st = h->cost_stats;
    });
}
