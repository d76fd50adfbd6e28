// The primal certificate's sparse correction (ipd_apd_set_correction): the deficits e, f of
// ipd_round.hip carried by a north-west-corner coupling along a row order sigma and a column order tau instead of the
// rank-one term e_i*f_j -- at most m + n - 1 entries (i, j, g), their cost without a walk over c, and the choice
// between the two forms on the device.  Reached from ipd_round.hip's stages under modes 1 and 2 only; mode 0 launches
// nothing of this unit.
//
//   scan     k_nw_scan, two workgroups (0 the columns, 1 the rows): Se and Sf in k_rd_last's shape, the masses
//            alpha_k = (p*e)[sigma_k]*Sf resp. beta_s = (q*f)[tau_s]*Se read through the order, coalesced, and their
//            inclusive prefixes in the header's shape -- thread c adds chunk c's NW_CHUNK masses in ascending order,
//            thread 0 adds the chunk totals in ascending order, thread c adds the offset of its chunk to its prefixes.
//            The workgroups also mark every dense slot empty.
//   merge    k_nw_merge, one thread per breakpoint of R u C.  A positive entry (k, s) ends at min(R_k, C_s): at the row
//            breakpoint k when R_k <= C_s, at the column breakpoint s otherwise.  The thread finds its partner by
//            binary search over the other prefix vector, forms w, g = w/(p_i*q_j), takes c_ij (class 2: and phi_ij)
//            through the workspace's cost source and writes (i, j, g, c*g, phi*g) into the dense slot
//            (k - 1) + (s - 1), which no other entry has (the entries form a staircase).
//   last     k_nw_last, one workgroup: the dense slots compacted into the list by an integer scan (thread t counts and
//            then copies the slots [t*span, (t + 1)*span), so the list ascends in (k, s)); cc and cp of the list in
//            Se's shape over the list order; everything k_rd_last does for the statistics; mode 2's choice; the scalars
//            for the writing kernels (those of pass W with t = 0 when the list carries the correction) and the
//            read-back's second part.
//   scatter  k_nw_scatter, one thread per list entry, after pass W wrote theta*X2: t*g added at (i, j) of up to three
//            destinations.  It reads ok and the count from the device as W does.
// Deterministic: fixed shapes, integer compaction, every (i, j) written by one thread -- no atomics of any kind.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ipd_apd_state.h"
#include "ipd_round_geo.h"
#include "ipd_round_nw_geo.h"
#include "ipd_walk_dev.h"

namespace {

static_assert(sizeof(NwInfoDev) == NW_INFO_DOUBLES * sizeof(double) && sizeof(RdDev) <= NW_DEV_DOUBLES * sizeof(double),
              "apd_nw_side sizes the results in doubles");
static_assert(NW_THREADS == 256 && NW_THREADS == TR, "the kernels are written for workgroups of 256 threads");

// ---------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------
struct NwScan {
    int m, n;
    const double* p;
    const double* q;
    const double* ef;        // [f (n); e (m)]
    const int32_t* sigma;    // nullptr: identity
    const int32_t* tau;
    double* pre;             // nw_pre_col, nw_pre_row
    int32_t* di;             // nw_slots entries, set to -1
};

__global__ __launch_bounds__(256) void k_nw_scan(const NwScan a) {
    __shared__ double red[APD_WAVES * 2];
    __shared__ double tot[NW_THREADS];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int m = a.m, n = a.n;
    double s[2] = {0.0, 0.0};   // Se, Sf: entries t, t + 256, ... per thread, then the tree, as k_rd_last
    for (int i = tid; i < m; i += NW_THREADS) {
        const double pe = a.p[i] * a.ef[n + i];
        s[0] += pe;
    }
    for (int j = tid; j < n; j += NW_THREADS) {
        const double qf = a.q[j] * a.ef[j];
        s[1] += qf;
    }
    walk_wave_sums(lane, wv, s, red);
    const double se = walk_waves_total<2>(red, 0), sf = walk_waves_total<2>(red, 1);
    const bool col = blockIdx.x == 0;
    const int len = col ? n : m;
    const int32_t* ord = col ? a.tau : a.sigma;
    const double* wt = col ? a.q : a.p;
    const double* dv = col ? a.ef : a.ef + n;
    const double other = col ? se : sf;
    double* pre = a.pre + (col ? nw_pre_col(0) : nw_pre_row(n, 0));   // pre[k], k = 0 .. len
    for (int k = tid; k < len; k += NW_THREADS) {
        const int at = ord ? ord[k] : k;
        const double wd = wt[at] * dv[at];
        pre[1 + k] = wd * other;
    }
    if (tid == 0) pre[0] = 0.0;
    const int slots = nw_slots(m, n);
    for (int k = blockIdx.x * NW_THREADS + tid; k < slots; k += 2 * NW_THREADS) a.di[k] = -1;
    __syncthreads();
    const int nch = nw_chunks(len);   // <= NW_THREADS: ipd_apd_set_correction refuses longer vectors
    const int k0 = tid * NW_CHUNK, k1 = min(k0 + NW_CHUNK, len);
    if (tid < nch) {
        double acc = 0.0;
        for (int k = k0; k < k1; ++k) {
            acc = acc + pre[1 + k];
            pre[1 + k] = acc;
        }
        tot[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double off = 0.0;
        for (int c = 0; c < nch; ++c) {
            const double t = tot[c];
            tot[c] = off;
            off = off + t;
        }
    }
    __syncthreads();
    if (tid > 0 && tid < nch) {   // chunk 0's offset is 0
        const double off = tot[tid];
        for (int k = k0; k < k1; ++k) pre[1 + k] = off + pre[1 + k];
    }
}

// ---------------------------------------------------------------------------
// merge
// ---------------------------------------------------------------------------
struct NwMerge {
    int m, n, cls2;
    const double* p;
    const double* q;
    const double* c;         // CostStored
    const double* phi;       // class 2
    const int32_t* sigma;
    const int32_t* tau;
    const double* pre;
    int32_t* di;
    int32_t* dj;
    double* dg;
    double* dc;
    double* dp;
};

// c(i, j) of the workspace's cost source: a gather of the stored entry, or the entry folded from the coordinates with
// the operations that would have stored it
__device__ __forceinline__ double nw_cost(const CostStored&, const double* c, int i, int j, int m) {
    return c[(size_t)j * m + i];
}
template <int D>
__device__ __forceinline__ double nw_cost(const CostFree<D>& cs, const double*, int i, int j, int) {
    double x[D], y[D];
    cost_src_row<D>(cs.s, i, x);
    cost_src_col<D>(cs.s, j, y);
    return cost_src_value<D>(cs.s, x, y);
}

template <class CS>
__global__ __launch_bounds__(256) void k_nw_merge(const NwMerge a, const CS cs) {
    const int b = blockIdx.x * NW_THREADS + threadIdx.x;   // breakpoint: the columns' first, then the rows'
    if (b >= a.n + a.m) return;
    const double* C = a.pre + nw_pre_col(0);      // C[0 .. n]
    const double* R = a.pre + nw_pre_row(a.n, 0);   // R[0 .. m]
    int k, s;
    double w;
    if (b < a.n) {   // the entry that ends at C_s: its row is the first k with R_k > C_s
        s = b + 1;
        const double hi = C[s], below = C[s - 1];
        if (!(hi > below)) return;   // no mass (or a NaN)
        int lo = 1, up = a.m + 1;
        while (lo < up) {
            const int mid = (lo + up) >> 1;   // 1 .. m
            if (R[mid] > hi)
                up = mid;
            else
                lo = mid + 1;
        }
        if (lo > a.m) return;   // C_s is not below the rows' total: the entry, if any, ends at a row breakpoint
        k = lo;
        const double rb = R[k - 1];
        const double from = rb > below ? rb : below;
        w = hi - from;
    } else {   // the entry that ends at R_k: its column is the first s with C_s >= R_k
        k = b - a.n + 1;
        const double hi = R[k], below = R[k - 1];
        if (!(hi > below)) return;
        int lo = 1, up = a.n + 1;
        while (lo < up) {
            const int mid = (lo + up) >> 1;   // 1 .. n
            if (C[mid] >= hi)
                up = mid;
            else
                lo = mid + 1;
        }
        if (lo > a.n) return;   // beyond the columns' total: rounding of the two totals
        s = lo;
        const double cb = C[s - 1];
        const double from = cb > below ? cb : below;
        w = hi - from;
    }
    if (!(w > 0.0)) return;
    const int i = a.sigma ? a.sigma[k - 1] : k - 1;
    const int j = a.tau ? a.tau[s - 1] : s - 1;
    const double pq = a.p[i] * a.q[j];
    const double g = w / pq;
    const double cv = nw_cost(cs, a.c, i, j, a.m);
    const double cg = cv * g;
    double pg = 0.0;
    if (a.cls2) pg = a.phi[(size_t)j * a.m + i] * g;
    const int slot = nw_slot(k, s);   // 0 .. m + n - 2
    a.di[slot] = i;
    a.dj[slot] = j;
    a.dg[slot] = g;
    a.dc[slot] = cg;
    a.dp[slot] = pg;
}

// ---------------------------------------------------------------------------
// last
// ---------------------------------------------------------------------------
struct NwLast {
    RdGeo g;
    int cls2, mode;
    double mu;
    const double* sA;    // the scalars of A, C and (mode 2) D: rd_scal_index
    const double* sC;
    const double* sD;
    const double* ab0;
    const double* ef;
    const double* b;
    const double* p;
    const double* q;
    const int32_t* di;
    const int32_t* dj;
    const double* dg;
    const double* dc;
    const double* dp;
    int32_t* li;
    int32_t* lj;
    double* lg;
    double* lc;
    double* lp;
    ipd_round_stats* out;
    RdDev* dev;
    RdDev* devw;
    NwInfoDev* info;
};

constexpr int NW_NSUM = 12;

// steps 9 to 12 of the header for one form's cc and cp
struct NwForm {
    double theta, t, fval;
    bool ok;
};
__device__ __forceinline__ NwForm nw_form(int cls2, double mu, double fs, double ms, double se, double sf, double cc,
                                          double cp) {
    NwForm r;
    r.theta = 1.0;
    if (!cls2) {
        r.t = se > 0.0 ? 1.0 / se : 0.0;
    } else if (ms >= mu) {
        r.theta = mu / ms;
        r.t = 0.0;
    } else {
        const double d = mu - ms;
        r.t = d / cp;
    }
    const double f1 = r.theta * fs;
    const double f2 = r.t * cc;
    r.fval = f1 + f2;
    r.ok = isfinite(r.theta) && isfinite(r.t) && isfinite(r.fval);
    if (cls2) {
        const double ts = r.t * se, tf = r.t * sf;
        r.ok = r.ok && ts <= 1.0 && tf <= 1.0;
    }
    return r;
}

__global__ __launch_bounds__(256) void k_nw_last(const NwLast a) {
    __shared__ double red[APD_WAVES * NW_NSUM];
    __shared__ int cnt[NW_THREADS];
    const RdGeo& g = a.g;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    // the list: the occupied slots in ascending order
    const int slots = nw_slots(g.m, g.n), span = nw_span(slots);
    const int s0 = min(tid * span, slots), s1 = min(s0 + span, slots);
    int mine = 0;
    for (int k = s0; k < s1; ++k) mine += a.di[k] >= 0 ? 1 : 0;
    cnt[tid] = mine;
    __syncthreads();
    int at = 0, count = 0;
    for (int t = 0; t < NW_THREADS; ++t) {
        const int c = cnt[t];
        at += t < tid ? c : 0;
        count += c;
    }
    for (int k = s0; k < s1; ++k) {
        const int i = a.di[k];
        if (i < 0) continue;
        a.li[at] = i;
        a.lj[at] = a.dj[k];
        a.lg[at] = a.dg[k];
        a.lc[at] = a.dc[k];
        a.lp[at] = a.dp[k];
        ++at;
    }
    __syncthreads();
    const int nblk = walk_blocks(g);
    // 0 .. 9 as k_rd_last (4, 5: the rank-one term's cc and cp, mode 2 only); 10, 11: the list's cc and cp
    double s[NW_NSUM];
#pragma unroll
    for (int k = 0; k < NW_NSUM; ++k) s[k] = 0.0;
    for (int k = tid; k < nblk; k += NW_THREADS) {
        s[0] += a.sA[(size_t)k * RD_NS + 0];
        s[1] += a.sA[(size_t)k * RD_NS + 1];
        s[2] += a.sC[(size_t)k * RD_NS + 0];
        s[3] += a.sC[(size_t)k * RD_NS + 1];
        if (a.mode == 2) {
            s[4] += a.sD[(size_t)k * RD_NS + 0];
            s[5] += a.sD[(size_t)k * RD_NS + 1];
        }
    }
    for (int i = tid; i < g.m; i += NW_THREADS) {
        const double pi = a.p[i];
        const double pe = pi * a.ef[g.n + i];
        s[6] += pe;
        const double d = a.ab0[g.n + i] - a.b[g.n + i];
        const double v = a.cls2 ? walk_pos(d) : fabs(d);
        const double pv = pi * v;
        s[7] += pv;
    }
    for (int j = tid; j < g.n; j += NW_THREADS) {
        const double qj = a.q[j];
        const double qf = qj * a.ef[j];
        s[8] += qf;
        const double d = a.ab0[j] - a.b[j];
        const double v = a.cls2 ? walk_pos(d) : fabs(d);
        const double qv = qj * v;
        s[9] += qv;
    }
    for (int k = tid; k < count; k += NW_THREADS) {
        s[10] += a.lc[k];
        s[11] += a.lp[k];
    }
    walk_wave_sums(lane, wv, s, red);
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < NW_NSUM; ++k) s[k] = walk_waves_total<NW_NSUM>(red, k);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        const double fs = s[2], ms = s[3], se = s[6], sf = s[8];
        const NwForm nw = nw_form(a.cls2, a.mu, fs, ms, se, sf, s[10], s[11]);
        NwForm use = nw;
        bool list = true;
        NwInfoDev info;
        info.cc[0] = info.cc[1] = info.fval[0] = info.fval[1] = nan;
        info.pad[0] = info.pad[1] = 0.0;
        if (a.mode == 2) {   // ok first, then the smaller value; the rank-one term stays on a tie
            const NwForm r1 = nw_form(a.cls2, a.mu, fs, ms, se, sf, s[4], s[5]);
            const double key_nw = a.cls2 ? nw.fval : s[10], key_r1 = a.cls2 ? r1.fval : s[4];
            list = (nw.ok && !r1.ok) || (nw.ok == r1.ok && key_nw < key_r1);
            if (!list) use = r1;
            info.cc[0] = s[4];
            info.cc[1] = s[10];
            info.fval[0] = r1.fval;
            info.fval[1] = nw.fval;
        }
        info.form = list ? 1 : 0;
        info.count = list ? count : 0;
        *a.info = info;
        ipd_round_stats st = {};
        st.fval = use.fval;
        st.fs = fs;
        st.cc = list ? s[10] : s[4];
        st.theta = use.theta;
        st.t = use.t;
        st.se = se;
        st.sf = sf;
        st.ms = a.cls2 ? ms : nan;
        st.cp = a.cls2 ? (list ? s[11] : s[5]) : nan;
        st.viol_in = s[7] + s[9];
        st.dropped = s[0];
        st.ndropped = (int64_t)s[1];
        st.ok = use.ok ? 1 : 0;
        *a.out = st;
        RdDev dv;
        dv.theta = use.theta;
        dv.t = use.t;
        dv.se = se;
        dv.sf = sf;
        dv.ok = use.ok ? 1 : 0;
        *a.dev = dv;
        if (list) dv.t = 0.0;   // pass W writes theta*X2, k_nw_scatter adds t*g
        *a.devw = dv;
    }
}

// ---------------------------------------------------------------------------
// scatter
// ---------------------------------------------------------------------------
struct NwScatter {
    int m, need_ok;
    const RdDev* dev;
    const NwInfoDev* info;
    const int32_t* li;
    const int32_t* lj;
    const double* lg;
    double* o0;   // destinations or nullptr; every one holds theta*X2
    double* o1;
    double* o2;
};

__global__ __launch_bounds__(256) void k_nw_scatter(const NwScatter a) {
    const int e = blockIdx.x * NW_THREADS + threadIdx.x;
    if (e >= a.info->count || (a.need_ok && !a.dev->ok)) return;
    const size_t idx = (size_t)a.lj[e] * a.m + a.li[e];
    const double tg = a.dev->t * a.lg[e];
    const double* src = a.o0 ? a.o0 : (a.o1 ? a.o1 : a.o2);
    const double xh = src[idx] + tg;
    if (a.o0) a.o0[idx] = xh;
    if (a.o1) a.o1[idx] = xh;
    if (a.o2) a.o2[idx] = xh;
}

bool is_permutation(const int32_t* ord, int len) {
    std::vector<char> seen((size_t)len, 0);
    for (int k = 0; k < len; ++k) {
        if (ord[k] < 0 || ord[k] >= len || seen[(size_t)ord[k]]) return false;
        seen[(size_t)ord[k]] = 1;
    }
    return true;
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
RoundNw apd_nw_side(ipd_apd* h, int side, NwInfoDev* info_dev) {
    Arena& S = *h->ctx->scratch;
    const size_t M = nw_list_cap(h->m, h->n);
    RoundNw w;
    w.pre = S.alloc<double>(nw_pre_len(h->m, h->n));
    w.di = S.alloc<int32_t>(M);
    w.dj = S.alloc<int32_t>(M);
    w.dg = S.alloc<double>(M);
    w.dc = S.alloc<double>(M);
    w.dp = S.alloc<double>(M);
    w.lc = S.alloc<double>(M);
    w.lp = S.alloc<double>(M);
    w.li = h->nw_i[side];
    w.lj = h->nw_j[side];
    w.lg = h->nw_g[side];
    w.devw = reinterpret_cast<RdDev*>(S.alloc<double>(NW_DEV_DOUBLES));
    w.info = info_dev ? info_dev : reinterpret_cast<NwInfoDev*>(S.alloc<double>(NW_INFO_DOUBLES));
    return w;
}

void apd_nw_rest(ipd_apd* h, const RoundShared& sh, const RoundSide& s) {
    hipStream_t stream = h->ctx->stream;
    const RoundNw& w = s.nw;
    const int32_t* sigma = h->corr_has_row ? h->corr_row : nullptr;
    const int32_t* tau = h->corr_has_col ? h->corr_col : nullptr;
    NwScan sc;
    sc.m = h->m;
    sc.n = h->n;
    sc.p = h->p;
    sc.q = h->q;
    sc.ef = s.ef;
    sc.sigma = sigma;
    sc.tau = tau;
    sc.pre = w.pre;
    sc.di = w.di;
    hipLaunchKernelGGL(k_nw_scan, dim3(2), dim3(NW_THREADS), 0, stream, sc);
    IPD_KERNEL_CHECK();
    NwMerge mg;
    mg.m = h->m;
    mg.n = h->n;
    mg.cls2 = h->cls == 2 ? 1 : 0;
    mg.p = h->p;
    mg.q = h->q;
    mg.c = h->c;
    mg.phi = h->phi;
    mg.sigma = sigma;
    mg.tau = tau;
    mg.pre = w.pre;
    mg.di = w.di;
    mg.dj = w.dj;
    mg.dg = w.dg;
    mg.dc = w.dc;
    mg.dp = w.dp;
    with_cost_source(h, [&](auto cs) {
        hipLaunchKernelGGL((k_nw_merge<decltype(cs)>), dim3(cdiv((long long)h->M, NW_THREADS)), dim3(NW_THREADS), 0,
                           stream, mg, cs);
    });
    IPD_KERNEL_CHECK();
    NwLast l;
    l.g = walk_make_geo(h->m, h->n);
    l.cls2 = mg.cls2;
    l.mode = h->corr_mode;
    l.mu = h->mu;
    l.sA = sh.sA;
    l.sC = s.sC;
    l.sD = s.sD;
    l.ab0 = sh.ab0;
    l.ef = s.ef;
    l.b = h->b;
    l.p = h->p;
    l.q = h->q;
    l.di = w.di;
    l.dj = w.dj;
    l.dg = w.dg;
    l.dc = w.dc;
    l.dp = w.dp;
    l.li = w.li;
    l.lj = w.lj;
    l.lg = w.lg;
    l.lc = w.lc;
    l.lp = w.lp;
    l.out = s.out;
    l.dev = static_cast<RdDev*>(s.dev);
    l.devw = w.devw;
    l.info = w.info;
    hipLaunchKernelGGL(k_nw_last, dim3(1), dim3(NW_THREADS), 0, stream, l);
    IPD_KERNEL_CHECK();
}

void apd_nw_scatter(ipd_apd* h, const RoundSide& s, int need_ok, double* o0, double* o1, double* o2) {
    NwScatter k;
    k.m = h->m;
    k.need_ok = need_ok;
    k.dev = static_cast<const RdDev*>(s.dev);
    k.info = s.nw.info;
    k.li = s.nw.li;
    k.lj = s.nw.lj;
    k.lg = s.nw.lg;
    k.o0 = o0;
    k.o1 = o1;
    k.o2 = o2;
    hipLaunchKernelGGL(k_nw_scatter, dim3(cdiv((long long)nw_slots(h->m, h->n), NW_THREADS)), dim3(NW_THREADS), 0,
                       h->ctx->stream, k);
    IPD_KERNEL_CHECK();
}

void apd_nw_record(ipd_apd* h, int side, const NwInfoDev* info) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    ipd_correction_info& c = h->corr_last;
    c.mode = h->corr_mode;
    c.form = info ? (int32_t)info->form : 0;
    c.count = info ? (int64_t)info->count : 0;
    for (int k = 0; k < 2; ++k) {
        c.cc[k] = info ? info->cc[k] : nan;
        c.fval[k] = info ? info->fval[k] : nan;
    }
    h->corr_last_side = side;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_apd_set_correction(ipd_apd* h, int32_t mode, const int32_t* row_order, const int32_t* col_order) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "ipd_apd_set_correction: NULL handle");
        IPD_REQUIRE(mode >= 0 && mode <= 2, IPD_E_ARG,
                    "ipd_apd_set_correction: mode must be 0 (rank-one), 1 (north-west) or 2 (the cheaper)");
        IPD_REQUIRE(!row_order || is_permutation(row_order, h->m), IPD_E_ARG,
                    "ipd_apd_set_correction: row_order is not a permutation of 0 .. m-1");
        IPD_REQUIRE(!col_order || is_permutation(col_order, h->n), IPD_E_ARG,
                    "ipd_apd_set_correction: col_order is not a permutation of 0 .. n-1");
        IPD_REQUIRE(mode == 0 || (h->m <= NW_MAX_LEN && h->n <= NW_MAX_LEN), IPD_E_LIMIT,
                    "ipd_apd_set_correction: the north-west correction takes m, n <= 16384");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        if (row_order) {
            if (!h->corr_row) h->corr_row = h->arena->alloc<int32_t>((size_t)h->m);
            ctx->upload(h->corr_row, row_order, (size_t)h->m);
        }
        if (col_order) {
            if (!h->corr_col) h->corr_col = h->arena->alloc<int32_t>((size_t)h->n);
            ctx->upload(h->corr_col, col_order, (size_t)h->n);
        }
        if (mode != 0 && !h->nw_g[0]) {
            const size_t M = nw_list_cap(h->m, h->n);
            for (int s = 0; s < 2; ++s) {
                h->nw_i[s] = h->arena->alloc<int32_t>(M);
                h->nw_j[s] = h->arena->alloc<int32_t>(M);
                h->nw_g[s] = h->arena->alloc<double>(M);
            }
        }
        ctx->sync();   // the uploads are complete before the caller's arrays may change
        h->corr_has_row = row_order != nullptr;
        h->corr_has_col = col_order != nullptr;
        h->corr_mode = mode;
    });
}

extern "C" int ipd_apd_correction_info(const ipd_apd* h, ipd_correction_info* out) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && out, IPD_E_ARG, "ipd_apd_correction_info: NULL argument");
        *out = h->corr_last;
    });
}

namespace {

// the first min(cap, count) entries of the last call's list through `copy(dst, src, bytes)`
template <class Copy>
void correction_entries(ipd_apd* h, int32_t* i, int32_t* j, double* g, int64_t cap, int64_t* count, Copy&& copy) {
    IPD_REQUIRE(h && count, IPD_E_ARG, "ipd_apd_correction_entries: NULL argument");
    IPD_REQUIRE(cap >= 0, IPD_E_ARG, "ipd_apd_correction_entries: cap must be >= 0");
    const int64_t have = h->corr_last.count;
    const size_t nn = (size_t)std::min<int64_t>(cap, have);
    const int s = h->corr_last_side;
    if (nn) {
        h->ctx->set_device();
        if (i) copy(i, h->nw_i[s], nn * sizeof(int32_t));
        if (j) copy(j, h->nw_j[s], nn * sizeof(int32_t));
        if (g) copy(g, h->nw_g[s], nn * sizeof(double));
        h->ctx->sync();
    }
    *count = have;
}

}  // namespace

extern "C" int ipd_apd_correction_entries(ipd_apd* h, int32_t* i, int32_t* j, double* g, int64_t cap, int64_t* count) {
    return ipd_guard([&] {
        correction_entries(h, i, j, g, cap, count,
                           [&](void* dst, const void* src, size_t bytes) { h->ctx->fetch_bytes(src, dst, bytes); });
    });
}

extern "C" int ipd_apd_correction_entries_dev(ipd_apd* h, int32_t* i_dev, int32_t* j_dev, double* g_dev, int64_t cap,
                                              int64_t* count) {
    return ipd_guard([&] {
        correction_entries(h, i_dev, j_dev, g_dev, cap, count, [&](void* dst, const void* src, size_t bytes) {
            IPD_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, h->ctx->stream));
        });
    });
}
