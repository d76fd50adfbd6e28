// Planner of the multi-launch path (amg_cycle, launch_top, the block solve: ipd_cycle.hip, ipd_block.hip): from
// the shapes of the levels and of their transfers, the device's CU count and three switches it decides, once per
// hierarchy, how every level's phases run -- lanes per row and grids of the row walks, the padded copy, LDS
// staging, which phases are queued into the fused single-workgroup program and which are launches of their own,
// whether residual and restriction run as one kernel.  amg_prepare_levels keeps what plan_launches returns; the
// launch code walks it and calls no rule.  Host-clean, no HIP, no getenv: tests/launch_plan_driver.cpp runs it
// on the CPU.
//
// Three things are not known here and stay decided at the launch: the mask form of level 1's sweeps
// (amg_attach_maskop), the root of the sub-cycle (the level planner's k_sub) and sharding over ranks (run_rows).
#pragma once

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "ipd_limits.h"

struct MatShape {
    int nr = 0, nc = 0, nnz = 0;
};
struct LaunchShape {   // level k and its transfers to level k + 1, as far as the rules look at them
    int nr = 0, nnz = 0;   // A_k
    int nf = 0;            // F-block size (level 1 of a bigraph hierarchy; 0 = Jacobi)
    int maxoff = 0;        // longest off-diagonal row (unused where the level's walk comes from a donor)
    MatShape Pt, P;        // k < J: P'_{k+1}, the restriction, and P_{k+1}, the prolongation
    bool t1 = false;       // T1 = P'_{k+1} A_k was kept
    MatShape T1;
};

struct LaunchSwitches {   // IPD_NO_PAD, IPD_NO_STAGE, IPD_NO_RRC (ipd_switches.h), read once per hierarchy
    bool no_pad = false, no_stage = false, no_rrc = false;
};

// lanes per row: about 2 entries per lane (half a ROW_U batch), widened while the launch
// would leave most of the chip idle
static inline int pick_lanes(long long nnz, int nrows, int blocks_target) {
    if (nrows <= 0) return 1;
    const double avg = (double)nnz / (double)nrows;
    int L = 1;  // short rows: one lane walks the whole row in a single ROW_U batch
    // mean entries per lane aimed at.  Short rows (the realistic levels): 2 -- m=n=1024 driver
    // runs, Class 1 / Class 2: 1.5: 1.54 / 0.75 s, 2: 1.52 / 0.73, 3: 1.55 / 0.75, 4: 1.61 / 0.80,
    // 6: 1.62 / 0.81.  Long rows (dense masks): 12 -- with 2 the 512..1024-entry rows of the
    // regime-D transfers spread over 512-1024 lanes and the cross-wave reduction costs more than
    // the shorter walk saves (k_xfer 6.6 -> 10.0 us, V cycle 0.200 -> 0.206 ms).
    const double forced = 0.0, forced_long = 0.0;
    // regime D, m=n=1024 / 2048, ms per V cycle: 3: 0.2007 / 0.387, 4.5: 0.1968 / 0.378,
    // 6: 0.1960 / 0.376, 9: 0.1975 / 0.374, 17: 0.1969 / 0.370
    // (with 512-thread blocks: 6: 0.1903 / 0.337, 12: 0.1866 / 0.324, 24: 0.1891 / 0.320)
    const double long_rows = forced_long > 0.0 ? forced_long : 3.0 * ROW_U;
    const double per_lane = forced > 0.0 ? forced : (avg >= 64.0 ? long_rows : 0.5 * ROW_U);
    while (L < BT && (double)L * per_lane < avg) L <<= 1;
    // widen while most of the chip would idle (tools/ubench_small.hip: a 1024-row launch of
    // short rows costs the same 6.5 us on 1, 4 or 16 workgroups, so spreading is free and
    // keeps one CU's load-issue rate from becoming the limit)
    while (L < BT && (long long)nrows * L < (long long)blocks_target * BT / 2 &&
           (double)L * 2.0 <= avg)
        L <<= 1;
    return L;
}

static inline int pick_blocks(int nrows, int L, int cu) {
    return (int)std::max<long long>(1, std::min<long long>(cu, ((long long)nrows * L + BT - 1) / BT));
}

// stride of a padded row: its longest off-diagonal row in whole 4-entry vectors
static inline int pad_stride(int maxoff) { return (maxoff + 3) / 4 * 4; }

// Width S of the padded off-diagonal copy of a level, 0 where it has none: the level is big and regular
// enough (see ipd_cycle_phases.h, item 2)
static inline int pad_width(int nr, int nnz, int maxoff /* longest off-diagonal row, from k_levels_prepare */) {
    if (nr > PAD_ROWS_MAX || nr == 0) return 0;
    const double avg_off = (double)(nnz - nr) / (double)nr;
    // small levels too: one dependent round trip less per launch (measured -6 % solve time on
    // the m=n=1024 Class 1 run)
    if (avg_off < PAD_AVG_MIN) return 0;
    const int S = pad_stride(maxoff);
    if (S == 0 || (double)S > PAD_SLACK_FACTOR * avg_off + PAD_SLACK) return 0;
    return S;
}

// Lanes per row of the padded walk: one batch (ROW_U entries = 2 vectors) per lane, widened until the chip is filled
static inline int padded_lanes(int S, int rows_per_launch, int cu) {
    const int nvec = S / 4;
    int L = 4;
    // batches per lane aimed at before the chip-filling rule below widens again.  Regime D at
    // m=n=2048 (2048-entry rows, bandwidth-bound): 1: 0.376 ms per V cycle, 2: 0.342, 4: 0.332,
    // 8/16: 0.332; m=n=1024 unchanged (0.197), m=n=4096 Class 1 run 5.37 -> 5.29 s
    // (with 512-thread blocks: 4: 0.337, 8: 0.324-0.330, 16: 0.325)
    const int batches = PAD_BATCHES;
    while (L < BT && L * (ROW_U / 4) * batches < nvec) L <<= 1;
    const double fill = 1.0;   // one workgroup per CU (0.5 left half the chip idle on a 1024-row level: 6.16 -> 5.79 us)
    while (L < BT && (double)rows_per_launch * L < fill * cu * BT && L < nvec) L <<= 1;
    return L;
}

// A gathered vector of `len` entries goes through LDS
static inline bool stage_fits(long long len) { return len <= STAGE_MAX; }
// ... the two vectors k_rrc gathers from (r and e of the fine level), on a level whose own walks are staged
static inline bool rrc_staged(int ncols, bool level_staged) { return stage_fits(2LL * ncols) && level_staged; }

// A phase is "small" when one workgroup covers its rows in ONE pass and its matrix slice
// is a few thousand entries: then it costs 1-3 us inside a fused program against >= 5 us
// as a launch of its own.  Larger phases lose inside a single workgroup (one CU issues
// ~60 B/clk of loads: tools/ubench_small.hip) and stay separate launches.
static inline bool phase_is_small(int rows, int L, double nnz_est, int stage_len) {
    return stage_len <= STAGE_MAX && (long long)rows * L <= (long long)BT && nnz_est <= QUEUED_NNZ_MAX;
}

// Residual and restriction as one kernel, r_{k+1} = P'r - (P'A) e (k_rrc), the fused-program case aside:
// fused where the two launches are latency-bound (measured: tree-mask W cycle 0.432 -> 0.413 ms,
// realistic Newton systems -2...-3.5 %); once T1 is megabytes the pair is bandwidth-bound and the
// fused walk (CSR T1, 12 B per entry, against the padded A, 10 B) is the slower one (regime D at
// m=n=2048: 0.321 -> 0.342 ms), so large T1 keep the two launches.
static inline bool rrc_applies(const LaunchShape& s, const LaunchSwitches& sw) {
    return !sw.no_rrc && s.t1 && s.T1.nr == s.Pt.nr && s.T1.nnz <= RRC_T1_NNZ_MAX;
}

struct RowRange {
    int r0 = 0, r1 = 0;   // rows [r0, r1)
    int G = 1;            // workgroups of their launch
};
// The row ranges of one smoother sweep, in order: a Jacobi level's rows (n == 1), or the two halves of the
// bigraph Gauss-Seidel level -- pre: F rows then C rows (Rk{1}); post: C rows then F rows (Rk{1}')
struct HalfRanges {
    int n = 0;
    RowRange r[2];
};
static inline HalfRanges half_ranges(int nf, int N, bool post) {
    HalfRanges h;
    h.n = nf > 0 ? 2 : 1;
    h.r[0].r1 = N;
    if (nf > 0) {
        h.r[0].r0 = post ? nf : 0, h.r[0].r1 = post ? N : nf;   // first half rows
        h.r[1].r0 = post ? 0 : nf, h.r[1].r1 = post ? nf : N;   // second half rows
    }
    return h;
}

struct XferPlan {   // a restriction or a prolongation
    int L = 1, G = 1;
    bool staged = false;   // the vector it gathers from goes through LDS
    bool queued = false;   // runs inside the fused program
};

struct LaunchLevel {   // how level k runs on the multi-launch path
    int N = 0, nf = 0;
    int lanes = 1;              // lanes per row of the CSR walk
    int S = 0, L = 1, G = 1;    // the launches' walk: pad width (0: the CSR arrays), lanes per row, workgroups of a sweep's launch
    int G_all = 1;              // workgroups of a walk of all rows (residual, top)
    bool staged = false;        // the level's vectors are gathered through LDS
    HalfRanges sweep[2];        // pre, post: the row ranges of a sweep (their grids: the rows kernel's)
    bool sweep_queued = false;
    // k < J
    bool resid_queued = false;
    XferPlan rest, prol;
    bool rrc_rule = false;      // k_rrc's rule holds, the fused-program case aside (what the block solve asks)
    bool rrc = false;           // ... and neither part is queued: residual + restriction are the one kernel
    XferPlan rrc_walk;          // its lanes, grid and staging (where rrc_rule holds)
    bool top_queued = false;    // k == 1: the top of the Class_AMG loop
    int pcg_L = 1;              // k == J: lanes per row of the coarsest level's PCG (always queued)
};

// `donor`: the records of levels 1..donor_levels (at most 2) of the hierarchy whose constant data this one
// shares, indexed by level; those levels take the donor's padded copy and the geometry that goes with it
inline std::vector<LaunchLevel> plan_launches(const LaunchShape* shapes, int J, int cu, const LaunchSwitches& sw,
                                              const LaunchLevel* donor = nullptr, int donor_levels = 0) {
    std::vector<LaunchLevel> plan((size_t)J + 1);
    // a transfer: rows of P' (coarse rows) gather the fine residual, rows of P (fine rows) the coarse correction
    auto xfer = [cu](const MatShape& m) {
        XferPlan x;
        x.L = pick_lanes(m.nnz, m.nr, cu);
        x.G = pick_blocks(m.nr, x.L, cu);
        x.staged = stage_fits(m.nc);
        x.queued = x.staged && phase_is_small(m.nr, x.L, (double)m.nnz, m.nc);
        return x;
    };
    for (int k = 1; k <= J; ++k) {
        const LaunchShape& s = shapes[k];
        LaunchLevel& p = plan[(size_t)k];
        const int N = p.N = s.nr;
        p.nf = s.nf;
        // launch geometry: for a GS level the work per launch is half the matrix
        const int rows_per_launch = s.nf > 0 ? std::max(1, N / 2) : N;
        const long long nnz_per_launch = s.nf > 0 ? std::max(1, s.nnz / 2) : s.nnz;
        p.lanes = p.L = pick_lanes(nnz_per_launch, rows_per_launch, cu);
        p.G = pick_blocks(rows_per_launch, p.L, cu);
        p.staged = stage_fits(N) && !sw.no_stage;
        if (donor && k <= 2 && k <= donor_levels) {
            p.S = donor[k].S;
            p.L = donor[k].L;
            p.G = donor[k].G;
            p.lanes = donor[k].lanes;
        } else if (!sw.no_pad && (p.S = pad_width(s.nr, s.nnz, s.maxoff)) > 0) {
            p.L = padded_lanes(p.S, rows_per_launch, cu);
            p.G = pick_blocks(rows_per_launch, p.L, cu);
        }
        p.G_all = pick_blocks(N, p.L, cu);
        const int rows_sweep = s.nf > 0 ? std::max(s.nf, N - s.nf) : N;
        p.sweep_queued = p.staged && phase_is_small(rows_sweep, p.L, (double)s.nnz * rows_sweep / std::max(N, 1), N);
        for (int post = 0; post < 2; ++post) {
            p.sweep[post] = half_ranges(s.nf, N, post != 0);
            for (RowRange& r : p.sweep[post].r) r.G = pick_blocks(r.r1 - r.r0, p.L, cu);
        }
        if (k == 1) p.top_queued = p.staged && phase_is_small(N, p.L, (double)s.nnz, N);
        if (k == J) {
            p.pcg_L = std::min(pick_lanes(s.nnz, s.nr, 1), PCG_LANES_MAX);
            continue;
        }
        p.resid_queued = p.staged && phase_is_small(N, p.L, (double)s.nnz, N);
        p.rest = xfer(s.Pt);
        p.prol = xfer(s.P);
        p.rrc_rule = rrc_applies(s, sw);
        p.rrc = p.rrc_rule && !p.resid_queued && !p.rest.queued;
        if (p.rrc_rule) {
            p.rrc_walk.L = pick_lanes((long long)s.T1.nnz + s.Pt.nnz, s.Pt.nr, cu);
            p.rrc_walk.G = pick_blocks(s.Pt.nr, p.rrc_walk.L, cu);
            p.rrc_walk.staged = rrc_staged(s.Pt.nc, p.staged);
        }
    }
    return plan;
}

// The record of level k as one line: what the planner's CPU test pins and IPD_DEBUG_LEVELS shows
static inline std::string launch_plan_line(const LaunchLevel& p, int k, int J) {
    std::string s;
    char b[128];
    auto add = [&](const char* fmt, auto... v) {
        std::snprintf(b, sizeof(b), fmt, v...);
        s += b;
    };
    auto how = [](bool queued) { return queued ? "queued" : "launched"; };
    add("level %d N=%d nf=%d lanes=%d S=%d L=%d G=%d G_all=%d staged=%d sweep=%s", k, p.N, p.nf, p.lanes, p.S, p.L, p.G,
        p.G_all, (int)p.staged, how(p.sweep_queued));
    for (int post = 0; post < 2; ++post) {
        add(" %s", post ? "post" : "pre");
        for (int i = 0; i < p.sweep[post].n; ++i) {
            const RowRange& r = p.sweep[post].r[i];
            add(" [%d,%d)x%d", r.r0, r.r1, r.G);
        }
    }
    if (k == 1) add(" top=%s", how(p.top_queued));
    if (k == J) {
        add(" pcg L=%d", p.pcg_L);
        return s;
    }
    if (p.rrc)
        s += " rrc";
    else
        add(" resid=%s", how(p.resid_queued));
    add(" rrc_rule=%d L=%d G=%d staged=%d", (int)p.rrc_rule, p.rrc_walk.L, p.rrc_walk.G, (int)p.rrc_walk.staged);
    add(" rest=%s L=%d G=%d staged=%d", how(p.rest.queued), p.rest.L, p.rest.G, (int)p.rest.staged);
    add(" prol=%s L=%d G=%d staged=%d", how(p.prol.queued), p.prol.L, p.prol.G, (int)p.prol.staged);
    return s;
}
