// The transport plan as a sparse matrix, out of and into the drivers' device workspace
// (ipd_apd_plan, ipd_apd_plan_dev, ipd_apd_set_plan).
//
// X = sparse(reshape(xk,m,n)) restricted to !(|x| <= tol), as m x n CSC with ascending rows, is
// built where xk lives: the dense iterate never crosses the host boundary, only the kept entries
// and n+1 column pointers do.
//
//   count   one streaming read of x and c.  Layout and walk are k_tiles' (ipd_apd_tiles.h):
//           x(i,j) = x[i + j*m], a wave owns 64 consecutive rows (one SEGMENT) and walks
//           16*reps columns alone, lanes along i (coalesced), 16 loads per lane and array in
//           flight, no LDS tile, no barrier inside the column loop.  The kept count of a
//           (column, segment) pair is a wave ballot and a population count; the sums of the
//           statistics leave as per-workgroup partials, the marginals Ax(x_kept) as the row /
//           column partials the driver's passes write (lpart / rpart): the geometry is the
//           driver's make_geo and the column butterfly is the tile walker's own.
//   offsets column-major order (columns outer, segments inner) in two levels: a wave per column
//           scans the column's segment counts in place and leaves the column total, and
//           exclusive_scan_i32 turns the n totals into the column pointers.  offset(j, seg) =
//           jc[j] + prefix(j, seg).  No workgroup waits for another one.
//   fill    a second read of x; the lane's position inside its segment is the population count
//           of the ballot below the lane, so rows come out ascending without a sort.  Indices
//           are 32-bit up to here and widened by the stores.
//
// Everything is deterministic: integer counts, partial sums that are added in a fixed order by
// the finishing kernel, no float atomics.
#pragma clang fp contract(off)

#include <cmath>
#include <cstdlib>

#include "ipd_apd_state.h"
#include "ipd_walk_dev.h"

namespace {

// TR, TC: ipd_apd_geo.h; colsum16, colsum_index: ipd_apd_tiles.h
constexpr int PSC = 4;    // statistics per workgroup: sum_kept, sum_dropped, max_dropped, fval_kept

struct PlanGeo {
    int m, n, nseg, nib, njg, reps;   // njg column groups of reps*TC columns
};

// the natural geometry of the driver's walker (IPD_APD_REPS is not read) plus the 64-row segments
PlanGeo plan_geo(int m, int n) {
    const Geo d = make_geo(m, n);
    PlanGeo g;
    g.m = m;
    g.n = n;
    g.nseg = cdiv(m, 64);
    g.nib = d.nib;
    g.njg = d.njg;
    g.reps = d.reps;
    return g;
}

// device-side results of the finishing kernel (read back in one piece)
struct PlanScal {
    double sum_kept, sum_dropped, max_dropped, fval_kept;
    long long nnz;
};

__device__ __forceinline__ double wave_add(double v) {   // butterfly: every lane ends with the same bits
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
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

// ---------------------------------------------------------------------------
// count pass
// ---------------------------------------------------------------------------
template <class CS>   // CS: CostStored or CostFree<D> (ipd_apd_tiles.h)
struct PlanCountT {
    PlanGeo g;
    const double* x;
    const double* c;   // CostStored
    const double* p;
    const double* q;
    double tol;
    int* cnt;        // [j * nseg + seg]
    double* spart;   // [workgroup][PSC]
    double* lpart;   // AX: [jg][m]      partial sums of X*q
    double* rpart;   // AX: [segment slot][n]  partial sums of X'*p (slots of absent segments hold zeros)
    [[no_unique_address]] CS cs;
};

template <bool AX, class CS>
__global__ __launch_bounds__(256) void k_plan_count(const PlanCountT<CS> a) {
    __shared__ double red[4 * PSC];
    const PlanGeo& g = a.g;
    const WalkLane t = walk_lane(g.m);   // on the driver's geometry: t.grp is its column group jg
    const int seg = t.slot();
    const double pi = (AX && t.in_i) ? a.p[t.i] : 0.0;
    typename CS::Row crow;
    a.cs.row(crow, t.ic);
    double skept = 0.0, sdrop = 0.0, mdrop = 0.0, fkept = 0.0, lacc = 0.0;
    for (int rep = 0; rep < g.reps; ++rep) {
        const int j0 = (t.grp * g.reps + rep) * TC;
        if (j0 >= g.n) break;  // uniform
        double xr[TC], cr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const size_t idx = walk_place(t, g, j0, jj);
            xr[jj] = a.x[idx];
            cr[jj] = CS::FREE ? 0.0 : a.c[idx];
        }
        // lane jj fetches q of column j0 + jj (16 uniform loads held 32 scalar registers too many)
        const double ql = (AX && t.lane < TC) ? a.q[min(j0 + t.lane, g.n - 1)] : 0.0;
        // matrix-free: and the coordinates of column j0 + (lane mod 16), for the same reason
        typename CS::Col clane;
        a.cs.col(clane, walk_lane_col(t, g, j0));
        int mycnt = 0;
        double xv[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const bool valid = t.in_i && j0 + jj < g.n;
            const double x = xr[jj];
            const double ab = fabs(x);
            const bool keep = valid && walk_keep(x, a.tol);
            const unsigned long long bal = __ballot(keep);
            if (t.lane == jj) mycnt = __popcll(bal);
            const double qj = AX ? __shfl(ql, jj) : 0.0;
            typename CS::Col ccol;
            a.cs.col_of_lane(ccol, clane, jj);
            double xk = 0.0;
            if (keep) {
                skept += x;
                fkept += a.cs.value(cr[jj], crow, ccol) * x;
                if (AX) lacc += x * qj;
                xk = x;
            } else if (valid) {
                sdrop += ab;
                mdrop = ab > mdrop ? ab : mdrop;
            }
            xv[jj] = xk * pi;
        }
        // lane jj holds the count of column j0 + jj: one store instruction for the 16 of them
        if (t.lane < TC && seg < g.nseg && j0 + t.lane < g.n) a.cnt[(size_t)(j0 + t.lane) * g.nseg + seg] = mycnt;
        if (AX) {
            const double cs = colsum16(xv, t.lane);
            int col;
            if (walk_col_owner(t, g, j0, col)) a.rpart[(size_t)seg * g.n + col] = cs;
        }
    }
    if (AX && t.in_i) a.lpart[(size_t)t.grp * g.m + t.i] = lacc;
    const double w0 = wave_add(skept), w1 = wave_add(sdrop), w2 = wave_max(mdrop), w3 = wave_add(fkept);
    if (t.lane == 0) {
        red[t.wv * PSC + 0] = w0;
        red[t.wv * PSC + 1] = w1;
        red[t.wv * PSC + 2] = w2;
        red[t.wv * PSC + 3] = w3;
    }
    __syncthreads();
    if (t.tid < PSC) {
        const int blk = t.grp * gridDim.x + t.ib;
        const double r0 = red[t.tid], r1 = red[PSC + t.tid], r2 = red[2 * PSC + t.tid], r3 = red[3 * PSC + t.tid];
        double r;
        if (t.tid == 2) {
            r = r0 > r1 ? r0 : r1;
            r = r2 > r ? r2 : r;
            r = r3 > r ? r3 : r;
        } else {
            r = r0 + r1 + r2 + r3;
        }
        a.spart[(size_t)blk * PSC + t.tid] = r;
    }
}

// ---------------------------------------------------------------------------
// offsets: a wave per column scans its segment counts in place (exclusive) and leaves the total
// ---------------------------------------------------------------------------
constexpr int SEG_PER_LANE = 4;   // nseg <= 16384 / 64 = 256 = 64 lanes x 4

__global__ __launch_bounds__(256) void k_plan_colscan(int n, int nseg, int* __restrict__ cnt,
                                                      int* __restrict__ colcnt) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;  // uniform per wave, no barrier below
    int* const row = cnt + (size_t)j * nseg;
    const int chunk = (nseg + 63) >> 6;
    const int b = min(nseg, lane * chunk), e = min(nseg, b + chunk);
    int v[SEG_PER_LANE];
    int s = 0;
#pragma unroll
    for (int k = 0; k < SEG_PER_LANE; ++k) {
        v[k] = b + k < e ? row[b + k] : 0;
        s += v[k];
    }
    int x = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    int run = x - s;
#pragma unroll
    for (int k = 0; k < SEG_PER_LANE; ++k) {
        if (b + k < e) row[b + k] = run;
        run += v[k];
    }
    if (lane == 63) colcnt[j] = x;
}

// ---------------------------------------------------------------------------
// finishing kernel: column pointers widened, marginals and statistics out of the partials
// ---------------------------------------------------------------------------
struct PlanFin {
    PlanGeo g;
    int nblk;
    const double* spart;
    const double* lpart;
    const double* rpart;
    const int* jc32;     // n+1
    int64_t* jc;         // n+1
    double* ax;          // n+m or NULL
    PlanScal* out;
};

// sum of `count` partials `stride` apart, in index order; the loads go out 8 at a time (the tile walker's
// sum_strided adds in the same order with 32 loads in flight)
__device__ __forceinline__ double sum_strided8(const double* __restrict__ base, int count, size_t stride) {
    double s = 0.0;
    int k = 0;
    for (; k + 8 <= count; k += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(k + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < count; ++k) s += base[(size_t)k * stride];
    return s;
}

__global__ __launch_bounds__(256) void k_plan_fin(const PlanFin a) {
    __shared__ double red[4 * PSC];
    const PlanGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int t = blockIdx.x * 256 + tid;
    if (t <= g.n) a.jc[t] = a.jc32[t];
    if (a.ax && t < g.n + g.m) {
        // [X'*p ; X*q]: the segment slots of a column, then the column groups of a row, in index order
        a.ax[t] = t < g.n ? sum_strided8(a.rpart + t, 4 * g.nib, (size_t)g.n)
                          : sum_strided8(a.lpart + (t - g.n), g.njg, (size_t)g.m);
    }
    if (blockIdx.x != 0) return;
    // the statistics: thread t adds workgroups t, t+256, ... in that order, then the 256 threads'
    // sums meet in a fixed tree -- the same bits on every run
    double acc[PSC] = {0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < a.nblk; b += 256) {
#pragma unroll
        for (int k = 0; k < PSC; ++k) {
            const double v = a.spart[(size_t)b * PSC + k];
            if (k == 2) acc[k] = v > acc[k] ? v : acc[k];
            else acc[k] += v;
        }
    }
#pragma unroll
    for (int k = 0; k < PSC; ++k) {
        const double w = k == 2 ? wave_max(acc[k]) : wave_add(acc[k]);
        if (lane == 0) red[wv * PSC + k] = w;
    }
    __syncthreads();
    if (tid == 0) {
        double r[PSC];
#pragma unroll
        for (int k = 0; k < PSC; ++k) {
            const double r0 = red[k], r1 = red[PSC + k], r2 = red[2 * PSC + k], r3 = red[3 * PSC + k];
            if (k == 2) {
                double mx = r0 > r1 ? r0 : r1;
                mx = r2 > mx ? r2 : mx;
                r[k] = r3 > mx ? r3 : mx;
            } else {
                r[k] = r0 + r1 + r2 + r3;
            }
        }
        a.out->sum_kept = r[0];
        a.out->sum_dropped = r[1];
        a.out->max_dropped = r[2];
        a.out->fval_kept = r[3];
        a.out->nnz = a.jc32[g.n];
    }
}

// ---------------------------------------------------------------------------
// fill pass
// ---------------------------------------------------------------------------
struct PlanFill {
    PlanGeo g;
    const double* x;
    double tol;
    const int* segpre;   // [j * nseg + seg]: kept entries of column j in the segments before seg
    const int* jc32;
    int64_t* ir;
    double* pr;
};

__global__ __launch_bounds__(256) void k_plan_fill(const PlanFill a) {
    const PlanGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int ib = blockIdx.x, jg = blockIdx.y;
    const int i = ib * TR + tid;
    const int seg = ib * 4 + wv;
    if (seg >= g.nseg) return;  // uniform per wave: a wave without rows (no barrier in this kernel)
    const bool in_i = i < g.m;
    const int ic = in_i ? i : g.m - 1;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int rep = 0; rep < g.reps; ++rep) {
        const int j0 = (jg * g.reps + rep) * TC;
        if (j0 >= g.n) break;  // uniform
        double xr[TC];
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const int j = min(j0 + jj, g.n - 1);
            xr[jj] = a.x[(size_t)j * g.m + ic];
        }
        int off = 0;   // lane jj: where the segment's entries of column j0 + jj start
        if (lane < TC) {
            const int j = min(j0 + lane, g.n - 1);
            off = a.jc32[j] + a.segpre[(size_t)j * g.nseg + seg];
        }
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
            const bool valid = in_i && j0 + jj < g.n;
            const double x = xr[jj];
            const bool keep = valid && walk_keep(x, a.tol);
            const unsigned long long bal = __ballot(keep);
            const int o = __shfl(off, jj);
            if (keep) {
                const size_t pos = (size_t)o + (size_t)__popcll(bal & below);
                a.ir[pos] = (int64_t)i;
                a.pr[pos] = x;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// scatter (set_plan): one thread per entry into the zeroed x block
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_plan_scatter(int m, int n, long long nnz, const int64_t* __restrict__ jc,
                                                      const int64_t* __restrict__ ir,
                                                      const double* __restrict__ pr, double* __restrict__ x) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nnz) return;
    // the entry's column: the last j with jc[j] <= t  (jc[0] = 0 <= t < nnz = jc[n])
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (jc[mid] <= t) lo = mid;
        else hi = mid;
    }
    x[(size_t)lo * m + (size_t)ir[t]] = pr[t];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct PlanWork {
    PlanGeo g;
    int* segpre = nullptr;
    int* jc32 = nullptr;
};

// count, offsets and the finishing kernel; *st is filled (the stream is waited for)
void plan_count_phase(ipd_apd* h, double tol, int64_t* jc_dev, double* ax_dev, PlanWork* wk,
                      ipd_plan_stats* st) {
    ipd_ctx* ctx = h->ctx;
    Arena& S = *ctx->scratch;
    // the counts and offsets are 32-bit; m, n <= 16384 (ipd_apd_create) keeps mn below 2^31
    IPD_REQUIRE(h->mn < (size_t(1) << 31), IPD_E_LIMIT, "ipd_apd_plan: 2^31 entries or more");
    const PlanGeo g = plan_geo(h->m, h->n);
    wk->g = g;
    const int nblk = g.nib * g.njg;
    int* cnt = S.alloc<int>((size_t)g.n * g.nseg);
    int* colcnt = S.alloc<int>((size_t)g.n);
    int* jc32 = S.alloc<int>((size_t)g.n + 1);
    double* spart = S.alloc<double>((size_t)nblk * PSC);
    PlanScal* dscal = reinterpret_cast<PlanScal*>(S.alloc<double>(sizeof(PlanScal) / sizeof(double)));
    double* lpart = nullptr;
    double* rpart = nullptr;
    if (ax_dev) {
        lpart = S.alloc<double>((size_t)g.njg * g.m);
        rpart = S.alloc<double>((size_t)g.nib * 4 * g.n);
    }
    with_cost_source(h, [&](auto cs) {
        PlanCountT<decltype(cs)> a;
        a.g = g;
        a.x = h->u;
        a.c = h->c;
        a.p = h->p;
        a.q = h->q;
        a.tol = tol;
        a.cnt = cnt;
        a.spart = spart;
        a.lpart = lpart;
        a.rpart = rpart;
        a.cs = cs;
        if (ax_dev)
            hipLaunchKernelGGL((k_plan_count<true, decltype(cs)>), dim3(g.nib, g.njg), dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL((k_plan_count<false, decltype(cs)>), dim3(g.nib, g.njg), dim3(256), 0, ctx->stream, a);
    });
    IPD_KERNEL_CHECK();
    hipLaunchKernelGGL(k_plan_colscan, dim3(cdiv(g.n, 4)), dim3(256), 0, ctx->stream, g.n, g.nseg, cnt, colcnt);
    IPD_KERNEL_CHECK();
    exclusive_scan_i32(ctx, colcnt, jc32, g.n);
    PlanFin f;
    f.g = g;
    f.nblk = nblk;
    f.spart = spart;
    f.lpart = lpart;
    f.rpart = rpart;
    f.jc32 = jc32;
    f.jc = jc_dev;
    f.ax = ax_dev;
    f.out = dscal;
    // n + m >= n + 1 threads: the column pointers and the marginals, one entry each
    hipLaunchKernelGGL(k_plan_fin, dim3(cdiv(g.n + g.m, 256)), dim3(256), 0, ctx->stream, f);
    IPD_KERNEL_CHECK();
    PlanScal s;
    ctx->fetch_bytes(dscal, &s, sizeof(PlanScal));
    st->nnz = (int64_t)s.nnz;
    st->sum_kept = s.sum_kept;
    st->sum_dropped = s.sum_dropped;
    st->max_dropped = s.max_dropped;
    st->fval_kept = s.fval_kept;
    IPD_REQUIRE(s.nnz >= 0 && (size_t)s.nnz <= h->mn, IPD_E_HIP, "ipd_apd_plan: the kept count is out of range");
    wk->segpre = cnt;
    wk->jc32 = jc32;
}

void plan_fill_phase(ipd_apd* h, double tol, const PlanWork& wk, int64_t* ir_dev, double* pr_dev) {
    PlanFill f;
    f.g = wk.g;
    f.x = h->u;
    f.tol = tol;
    f.segpre = wk.segpre;
    f.jc32 = wk.jc32;
    f.ir = ir_dev;
    f.pr = pr_dev;
    hipLaunchKernelGGL(k_plan_fill, dim3(wk.g.nib, wk.g.njg), dim3(256), 0, h->ctx->stream, f);
    IPD_KERNEL_CHECK();
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_plan_dev(ipd_apd* h, double tol, int64_t cap, int64_t* jc_dev, int64_t* ir_dev,
                                double* pr_dev, ipd_plan_stats* st, double* ax_dev) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && st && jc_dev, IPD_E_ARG, "ipd_apd_plan_dev: NULL argument");
        IPD_REQUIRE(tol >= 0.0, IPD_E_ARG, "ipd_apd_plan_dev: tol must be >= 0");   // false for a NaN
        IPD_REQUIRE(cap >= 0, IPD_E_ARG, "ipd_apd_plan_dev: cap must be >= 0");
        IPD_REQUIRE(cap == 0 || (ir_dev && pr_dev), IPD_E_ARG, "ipd_apd_plan_dev: ir_dev / pr_dev are NULL");
        CallScope scope(h->ctx);
        PlanWork wk;
        plan_count_phase(h, tol, jc_dev, ax_dev, &wk, st);
        if (st->nnz > cap) {
            h->ctx->sync();
            throw IpdError(IPD_E_LIMIT, "ipd_apd_plan_dev: the plan has " + std::to_string(st->nnz) +
                                            " entries, cap is " + std::to_string(cap));
        }
        if (st->nnz > 0) plan_fill_phase(h, tol, wk, ir_dev, pr_dev);
        h->ctx->sync();   // the scratch arrays are the next call's
    });
}

extern "C" int ipd_apd_plan(ipd_apd* h, double tol, ipd_csc_out* X, ipd_plan_stats* st, double* ax) {
    if (X) {
        X->nrows = X->ncols = X->nnz = 0;
        X->jc = X->ir = nullptr;
        X->pr = nullptr;
    }
    const int rc = ipd_guard([&] {
        IPD_REQUIRE(h && X && st, IPD_E_ARG, "ipd_apd_plan: NULL argument");
        IPD_REQUIRE(tol >= 0.0, IPD_E_ARG, "ipd_apd_plan: tol must be >= 0");   // false for a NaN
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        Arena& S = *ctx->scratch;
        const int M = h->m + h->n;
        int64_t* jc_dev = S.alloc<int64_t>((size_t)h->n + 1);
        double* ax_dev = ax ? S.alloc<double>((size_t)M) : nullptr;
        PlanWork wk;
        plan_count_phase(h, tol, jc_dev, ax_dev, &wk, st);
        const size_t nnz = (size_t)st->nnz;
        X->jc = (int64_t*)std::malloc(sizeof(int64_t) * ((size_t)h->n + 1));
        X->ir = (int64_t*)std::malloc(sizeof(int64_t) * (nnz ? nnz : 1));
        X->pr = (double*)std::malloc(sizeof(double) * (nnz ? nnz : 1));
        if (!X->jc || !X->ir || !X->pr) throw IpdError(IPD_E_NOMEM, "out of host memory");
        if (nnz) {
            int64_t* ir_dev = S.alloc<int64_t>(nnz);
            double* pr_dev = S.alloc<double>(nnz);
            plan_fill_phase(h, tol, wk, ir_dev, pr_dev);
            ctx->fetch(ir_dev, X->ir, nnz);
            ctx->fetch(pr_dev, X->pr, nnz);
        }
        ctx->fetch(jc_dev, X->jc, (size_t)h->n + 1);
        if (ax) ctx->fetch(ax_dev, ax, (size_t)M);
        X->nrows = h->m;
        X->ncols = h->n;
        X->nnz = st->nnz;
    });
    if (rc != IPD_OK && X) ipd_csc_free(X);
    return rc;
}

extern "C" int ipd_apd_set_plan(ipd_apd* h, const ipd_csc* X) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && X, IPD_E_ARG, "ipd_apd_set_plan: NULL argument");
        // everything is checked on the host before the workspace is touched
        IPD_REQUIRE(X->nrows == h->m && X->ncols == h->n, IPD_E_ARG, "ipd_apd_set_plan: X must be m x n");
        IPD_REQUIRE(X->nnz >= 0 && X->jc && (X->nnz == 0 || (X->ir && X->pr)), IPD_E_ARG,
                    "ipd_apd_set_plan: NULL array or negative nnz");
        IPD_REQUIRE(X->jc[0] == 0, IPD_E_ARG, "ipd_apd_set_plan: jc[0] must be 0");
        for (int j = 0; j < h->n; ++j)
            IPD_REQUIRE(X->jc[j + 1] >= X->jc[j], IPD_E_ARG, "ipd_apd_set_plan: jc must be non-decreasing");
        IPD_REQUIRE(X->jc[h->n] == X->nnz, IPD_E_ARG, "ipd_apd_set_plan: jc[n] must be nnz");
        for (int j = 0; j < h->n; ++j) {
            int64_t prev = -1;
            for (int64_t t = X->jc[j]; t < X->jc[j + 1]; ++t) {
                const int64_t r = X->ir[t];
                IPD_REQUIRE(r >= 0 && r < h->m, IPD_E_ARG, "ipd_apd_set_plan: row index outside [0, m)");
                IPD_REQUIRE(r > prev, IPD_E_ARG, "ipd_apd_set_plan: rows must be strictly ascending in a column");
                prev = r;
            }
        }
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        const size_t nnz = (size_t)X->nnz;
        if (nnz) {
            Arena& S = *ctx->scratch;
            int64_t* jc_dev = S.alloc<int64_t>((size_t)h->n + 1);
            int64_t* ir_dev = S.alloc<int64_t>(nnz);
            double* pr_dev = S.alloc<double>(nnz);
            ctx->upload(jc_dev, X->jc, (size_t)h->n + 1);
            ctx->upload(ir_dev, X->ir, nnz);
            ctx->upload(pr_dev, X->pr, nnz);
            IPD_HIP(hipMemsetAsync(h->u, 0, h->mn * sizeof(double), ctx->stream));
            hipLaunchKernelGGL(k_plan_scatter, dim3(cdiv((long long)nnz, 256)), dim3(256), 0, ctx->stream, h->m,
                               h->n, (long long)nnz, jc_dev, ir_dev, pr_dev, h->u);
            IPD_KERNEL_CHECK();
        } else {
            IPD_HIP(hipMemsetAsync(h->u, 0, h->mn * sizeof(double), ctx->stream));
        }
        IPD_HIP(hipMemcpyAsync(h->v, h->u, h->mn * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        ctx->sync();   // the scratch arrays are the next call's
        apd_restart_script(h);
    });
}
