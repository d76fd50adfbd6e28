// Planner of the resident kernels (ipd_resident.h, ipd_resident_big.h): from the level shapes, the
// options, the switches, the device's CU count and the LDS images the level plan packed it decides
// which resident mode a hierarchy runs -- none, k_resident, the mask-form kernel's three-level or deep
// mode --, which instantiation, how many workgroups, which tail.  ipd_resident_host.hip does the device work a
// plan calls for and commits it.  Host-clean, no HIP, no getenv: tests/resident_plan_driver.cpp runs it
// on the CPU.
//
// The decision is taken at three moments, in this order: plan_resident at amg_prepare_levels, and at
// amg_attach_maskop (once the bit mask of level 1 is there) plan_resident_big and plan_resident_deep.
#pragma once

#include <tuple>

#include "ipd_level_plan.h"

enum ResidentKind { RESIDENT_NONE, RESIDENT_K, RESIDENT_BIG, RESIDENT_DEEP };

// The template arguments of an instantiation: k_resident<ke, ke, ke3, poly2> or k_resident_big<ke2, rpw, deep>
struct ResidentKey {
    bool big = false;
    int ke = 0, ke3 = 0;   // k_resident: entries per lane of a padded row of levels 1-2 / of level 3 (0: not resident, 1: polynomial form)
    bool poly2 = false;    // ... level 2 composed over a visit (ipd_amg_attach_level2_poly)
    int ke2 = 0, rpw = 0;  // k_resident_big: entries per lane of a level-2 row, rows of a block per wave
    bool deep = false;
    bool full = false;     // k_resident, poly2: the full-shape form (resident_takes_full)
    static ResidentKey k(int ke, int ke3, bool poly2) { return ResidentKey{false, ke, ke3, poly2, 0, 0, false}; }
    static ResidentKey mask(int ke2, int rpw, bool deep) { return ResidentKey{true, 0, 0, false, ke2, rpw, deep}; }
    bool operator==(const ResidentKey& o) const {
        return std::tie(big, ke, ke3, poly2, ke2, rpw, deep, full) ==
               std::tie(o.big, o.ke, o.ke3, o.poly2, o.ke2, o.rpw, o.deep, o.full);
    }
};

struct ResidentImage {   // an LDS image a tail workgroup can take
    bool have = false;
    size_t lds = 0;      // its dynamic LDS
    size_t bm = 0;       // ... and what its operator copy needs on top (SolveDesc::bm_src; 0: none)
};

struct ResidentInputs {
    const LevelShape* L = nullptr;   // 1..J
    int J = 0;
    int S[4] = {0, 0, 0, 0};         // levels 1..3: stride of the launches' padded copy, 0 = none
    char cycle = 'v';
    int smoth = 1;
    bool twogrid = false, bigph = false;
    int num_cu = 256;
    bool small_ok = false;           // the whole solve is the single-workgroup one
    int k_sub = 0;                   // root of the IMG_SUB image
    ResidentImage img[IMG_NONE];     // by role: IMG_SUB, IMG_SUB3, IMG_SUB4
    ImageRole sub5 = IMG_NONE;       // the image that serves a tail rooted at level 5 (LevelPlan::sub5)
    bool cyc() const { return cycle == 'w' || cycle == 'v'; }
    bool have5() const { return sub5 != IMG_NONE && img[sub5].have; }
    int rows(int k) const { return k <= J ? L[k].nr : 0; }
};

// What only the hierarchy's history and the device can tell the planners of amg_attach_maskop
struct ResidentFacts {
    int m, n;          // the mask's dimensions (C and F block of level 1)
    bool off;          // IPD_NO_RESIDENT=1 when the hierarchy was set up
    bool ok;           // a resident plan is active
    bool mask_form;    // a mask-form plan was committed (active or given up since)
    bool wident;       // the active k_resident plan's transfers are P = [W; I] (verified)
};

struct ResidentPlan {
    ResidentKind kind = RESIDENT_NONE;
    bool considered = false;   // plan_resident got as far as looking at the rows (the "[ipd] resident plan:" line)
    ResidentKey key;
    int G = 0;                 // resident workgroups
    size_t lds = 0;            // dynamic LDS of the launch
    bool remote = false;       // levels below the resident ones served by a tail workgroup (else: local tail)
    bool three = false;        // k_resident: level 3 resident as well
    bool poly3 = false, poly4 = false;   // level 3 / levels 3 and 4 in polynomial form
    int tail_root = 0;         // level the tail is rooted at (3, 4, 5)
    int Nin = 0;               // k_resident: rows of the remote tail's root level / of the local tail
    ImageRole tail_image = IMG_NONE;   // the remote tail's LDS image
    bool tail_bm = false;      // ... with room for its operator copy
    int S[4] = {0, 0, 0, 0};   // levels 1..3: stride of the rows the kernel loads
    bool priv[4] = {false, false, false, false};   // ... from a private padded copy (the launches have none)
    int wident = 0;            // k_resident, P = [W; I]: 1 by construction, 0 no, -1 to be checked on the device
    int ranks = 1;             // mask-form three-level mode: rank groups with a granule buffer each
    int levels = 0;            // what ipd_amg_resident_levels reports: levels held by the resident workgroups

    int grid() const { return G + (remote ? 1 : 0); }
};

static inline int resident_cdiv(int a, int b) { return (a + b - 1) / b; }

// stride of level k's rows in a resident kernel: the launches' padded copy, or -- rows live in registers, the
// padded stride is only a layout there -- for a level whose rows are too uneven for that copy (hubs) a private
// copy with its longest row as stride (built once the hierarchy is known to be taken)
static inline int resident_stride(const ResidentInputs& in, int k, bool* priv) {
    *priv = in.S[k] <= 0 && in.L[k].maxoff > 0;
    return *priv ? pad_stride(in.L[k].maxoff) : in.S[k];
}

// ---- level-resident kernel (k_resident) ----------------------------------------------------
// Eligible: three levels -- a bigraph Gauss-Seidel level 1 and a Jacobi level 2 with padded
// rows of at most 1024 entries, at most 2048 rows each, and a tail level of at most 64 rows --
// i.e. the dense regimes (regime D), where each launch of the multi-launch path is
// latency-bound.  IPD_NO_RESIDENT=1 switches it off, IPD_RESIDENT_G overrides the grid.
inline ResidentPlan plan_resident(const ResidentInputs& in, const PlanSwitches& sw) {
    ResidentPlan p;   // (kind RESIDENT_NONE until the last check has passed)
    if (sw.no_resident) return p;
    if (in.small_ok || in.J < 3 || in.twogrid) return p;
    p.considered = true;
    p.S[1] = resident_stride(in, 1, &p.priv[1]);
    p.S[2] = resident_stride(in, 2, &p.priv[2]);
    const int N1 = in.L[1].nr, N2 = in.L[2].nr, Nt = in.L[3].nr, nf = in.L[1].nf, nc = N1 - nf;
    const int N4 = in.rows(4);
    if (nf <= 0 || nc <= 0 || p.S[1] <= 0 || p.S[2] <= 0) return p;
    if (N1 > 4 * BT || N2 > 4 * BT || nf > 2 * BT || nc > 2 * BT || Nt < 1) return p;
    // everything below level 2: a tail of <= 64 rows solved redundantly by every workgroup (three
    // levels), or -- deeper hierarchies -- the single-workgroup sub-cycle rooted at level 3 run by ONE
    // extra workgroup out of its LDS image (the image the multi-launch path launches k_subcycle with)
    const bool local_tail = in.J == 3 && Nt <= RES_TAIL_MAX;
    bool remote = false, three = false;
    int ke3 = 0;
    ImageRole tail = IMG_NONE;   // the remote tail's LDS image
    if (!local_tail) {
        const bool cyc = in.cyc();
        remote = !sw.no_resident_remote && in.J >= 4 && Nt <= BT && cyc &&
                 ((in.k_sub == 3 && in.img[IMG_SUB].have) || (in.k_sub == 0 && in.img[IMG_SUB3].have));
        // Level 3 in the registers of the resident workgroups as well, the tail rooted at level 4: for
        // a level 3 too big for the tail's LDS (a few hundred rows of 15-100 entries), and preferred to
        // the tail rooted at level 3 whenever an image rooted at level 4 exists (the tail's legs are the
        // serial part of a cycle: ~22 us each from level 4, ~100 us from level 3).
        tail = in.k_sub == 0 ? IMG_SUB3 : IMG_SUB;
        const bool img4 = (in.k_sub == 4 && in.img[IMG_SUB].have) || (in.k_sub == 3 && in.img[IMG_SUB4].have);
        // level 3 fits the resident workgroups' registers: its rows (usually too uneven for the launches'
        // padded copy -- hubs -- but in registers the stride is only a layout: a private copy with the
        // longest row as stride), the row slots and a root level 4 of at most BT rows
        bool priv3 = false;
        const int S3 = resident_stride(in, 3, &priv3);
        const bool three_fits = in.J >= 4 && S3 > 0 && S3 <= 512 && Nt <= BT && N4 <= BT && N2 <= RES_NMAX / 2 &&
                                std::max(p.S[1], p.S[2]) <= 512 && Nt + resident_rows_G(nf, nc, N2) <= 2 * BT;
        if (!sw.no_resident_remote && !sw.no_resident_three && in.J >= 5 && img4 && cyc) {
            if (three_fits) {
                three = remote = true;
                ke3 = S3 <= 256 ? 4 : 8;
                if (in.k_sub == 3) tail = IMG_SUB4;
            }
        }
        // Four levels with a level 3 too big for any LDS image and a coarsest level of at most 64 rows
        // (dense masks early in a run, the bench's tree / hub masks): level 3 resident, level 4 solved
        // by every workgroup as the local tail -- no tail workgroup.
        // (a V cycle visits the tail once: there the local tail stays ahead of a tail workgroup rooted at a
        // level 3 in block-wide polynomial form -- tree mask 0.096 against 0.102 ms; a W cycle is the other
        // way round, 0.198 against 0.191)
        if (remote && !three && in.J == 4 && in.cycle == 'v' && !sw.no_resident_three && N4 <= RES_TAIL_MAX &&
            three_fits)
            remote = false;
        if (!remote && !sw.no_resident_remote && !sw.no_resident_three && in.J == 4 && cyc && N4 <= RES_TAIL_MAX &&
            three_fits) {
            three = true;
            ke3 = S3 <= 256 ? 4 : 8;
        }
        if (!remote && !three) return p;
        p.S[3] = S3;
    }
    const int smax = std::max(p.S[1], p.S[2]);
    int ke = 4;
    while (64 * ke < smax) ke <<= 1;
    if (ke > 16) return p;
    if (three && ke > 8) return p;   // (the third row slice does not fit beside two 16-entry ones)
    int G = resident_rows_G(nf, nc, N2);
    G = std::max(G, sw.resident_g);
    // every workgroup owns at least one row of every block (the hand-off protocol needs it)
    if (G + (remote ? 1 : 0) > in.num_cu || G > std::min(std::min(nf, nc), N2)) return p;
    const int Nin = three ? N4 : Nt;   // rows of the remote tail's root level / of the local tail
    if (remote && Nin > RES_WAVES * G) return p;   // one row of the restriction to it per wave
    if (three && Nt + G > 2 * BT) return p;        // level-3 hand-offs: N3 + G granules, two per thread
    // level 3 in polynomial form (ResDesc::p3rows): remote tail, one restriction row per workgroup at most,
    // at most four rows of level 3 per workgroup
    const bool poly3 = three && remote && in.smoth >= 1 && resident_poly3_root_fits(N4, G) && Nt <= 4 * G && Nt <= BT &&
                       !sw.no_poly;
    if (poly3) ke3 = 1;
    // level 4 resident as well (ResDesc::p4rows), the tail workgroup rooted at level 5
    const int N5r = in.J >= 6 ? in.L[5].nr : 0;
    const bool poly4 = poly3 && in.have5() && N1 <= RES_NMAX && N5r >= 1 && N5r <= 64 && N5r <= G &&
                       N4 <= RES_P4_SEG && N4 + G <= BT;
    size_t tail_lds = remote ? in.img[tail].lds : 0, tail_bm = remote ? in.img[tail].bm : 0;
    if (poly4) {
        tail = in.sub5;
        tail_lds = in.img[tail].lds;
        tail_bm = 0;   // (entered at level 5: the copied level is one the resident workgroups hold)
    }
    if (!remote || tail_lds + tail_bm > RES_LDS_MAX) tail_bm = 0;
    const size_t lds = remote ? std::max<size_t>(RES_LDS_BYTES, tail_lds + tail_bm) : RES_LDS_BYTES;
    if (lds > RES_LDS_MAX) return p;
    p.kind = RESIDENT_K;
    p.key = ResidentKey::k(ke, ke3, false);
    p.G = G;
    p.lds = lds;
    p.remote = remote;
    p.three = three;
    p.poly3 = poly3;
    p.poly4 = poly4;
    p.tail_root = poly4 ? 5 : three ? 4 : 3;
    p.Nin = Nin;
    p.tail_image = remote ? tail : IMG_NONE;
    p.tail_bm = remote && tail_bm > 0;
    p.priv[3] = three && !poly3 && in.S[3] <= 0;   // (the polynomial form does not read the rows)
    // bigraph transfers P = [W; I]: the kernel adds the identity entries instead of walking them
    // (a bigraph level 1 built by amg_transfer has them by construction -- k_bigph_fill writes the rows of I --
    // which saves the check and its round trip on every hierarchy of a run)
    p.wident = N2 != nc ? 0 : in.bigph ? 1 : -1;
    p.levels = poly4 ? 4 : ke3 > 0 ? 3 : 2;
    return p;
}

// Level 2 of k_resident in polynomial form, composed over a whole visit (ResDesc::p2rows): three levels with a
// one-row tail, V cycle, 16-entry slices -- the metric's workload (amg_attach_poly2 packs it on request)
inline bool resident_takes_poly2(const ResidentPlan& p, const ResidentInputs& in) {
    if (p.kind != RESIDENT_K || p.key.poly2 || p.remote || p.key.ke3 != 0 || p.key.ke != 16) return false;
    return in.J == 3 && p.Nin == 1 && !p.three && in.cycle == 'v' && in.smoth >= 1 && in.L[2].nr <= RES_NMAX / 2 &&
           in.L[1].nf <= RES_NMAX / 2 && in.L[2].nr <= 64 * 16;
}

// What the attach calls and the options have left in the descriptor of a k_resident plan
struct ResidentFullFacts {
    bool mask_transfers;   // level 1 <-> 2 transfers from the bit mask are attached (ResDesc::xm)
    int wident;            // P = [W; I]: 1 yes (by construction or verified), 0 no, -1 not verified yet
    int isnsp;
    bool localfirst;       // zero-start first sweeps are formed locally (ResDesc::localfirst)
};

// The full-shape form of the composed instantiation (k_resident's FULL): the metric's shape, where every size, row
// range and mode flag of the kernel is a constant -- F block, C block and level 2 of 2 BT rows each, RES_WAVES rows of
// every block per workgroup, transfers from the mask with P = [W; I], isnsp, local first sweeps, at least one sweep,
// a one-row local tail and the V cycle (the last two: resident_takes_poly2).  IPD_RES_NO_FULL=1 keeps the general form.
inline bool resident_takes_full(const ResidentPlan& p, const ResidentInputs& in, const ResidentFullFacts& f,
                                const PlanSwitches& sw) {
    if (sw.res_no_full || p.kind != RESIDENT_K || !p.key.poly2 || p.key.ke != 16 || p.key.ke3 != 0 || p.remote || p.three)
        return false;
    if (in.J != 3 || p.Nin != 1 || in.cycle != 'v' || in.smoth < 1) return false;
    const int nf = in.L[1].nf, nc = in.L[1].nr - nf, N2 = in.L[2].nr;
    if (nf != 2 * BT || nc != 2 * BT || N2 != 2 * BT || p.G * RES_WAVES != nf) return false;
    return f.mask_transfers && f.wident == 1 && f.isnsp == 1 && f.localfirst;
}

// ---- mask-form kernel (k_resident_big), planned once the bit mask of level 1 is there -------
// the level-resident kernel takes its level 1 <-> 2 transfers from the mask whatever the size ...
inline bool resident_wants_mask_transfers(const ResidentInputs& in, const ResidentFacts& f) {
    return f.ok && f.wident && in.J == 3;
}
// ... where its blocks have the mask's shape
inline bool resident_mask_transfers_fit(const ResidentInputs& in, const ResidentFacts& f) {
    return in.L[1].nf <= RES_NMAX / 2 && in.L[2].nr == f.m;
}

// Level 1 beyond k_resident's 2048 rows (m = n = 2048: BASELINE config 4's size), three levels with a
// one-row tail: the mask-form resident kernel (ipd_resident_big.h).  IPD_RESIDENT_BIG=1 prefers it
// wherever it applies (tests) -- it then replaces a k_resident plan --, IPD_NO_RESIDENT_BIG=1 switches it off.
inline ResidentPlan plan_resident_big(const ResidentInputs& in, const PlanSwitches& sw, const ResidentFacts& f) {
    ResidentPlan p;
    const int n = f.n, m = f.m;
    const int G = resident_cdiv(std::max(n, m), RES_WAVES);
    if (!(!sw.no_resident && !f.off && !sw.no_resident_big && (sw.resident_big || (!f.ok && n + m > RES_NMAX)) &&
          !in.small_ok && !f.mask_form && in.J == 3 && in.L[3].nr == 1 && n <= RB_HALF && m <= RB_HALF &&
          in.L[2].nr == m && in.cyc() && !in.twogrid && G <= in.num_cu && G <= std::min(n, m) && in.smoth >= 1))
        return p;
    p.S[2] = resident_stride(in, 2, &p.priv[2]);
    if (!(p.S[2] > 0 && p.S[2] <= 64 * 32)) return p;
    p.kind = RESIDENT_BIG;
    p.key = ResidentKey::mask(p.S[2] <= 64 * 16 ? 16 : 32, 1, false);
    p.G = G;
    p.lds = RB_LDS_BYTES;
    p.tail_root = 3;
    p.levels = 2;
    p.ranks = std::max(1, std::min(8, sw.resident_ranks));   // (test hook, see ResBigDesc::ranks)
    if (p.ranks > G) p.ranks = 1;
    return p;
}

// the image of the deep mode's tail workgroup, rooted at level 4 (rooted at 5: POLY4 only)
static inline ImageRole resident_deep_image(const ResidentInputs& in) {
    if ((in.k_sub == 4 && in.img[IMG_SUB].have) || (in.k_sub == 5 && in.have5())) return IMG_SUB;
    if (in.k_sub == 3 && in.img[IMG_SUB4].have) return IMG_SUB4;
    return IMG_NONE;
}

// Realistic hierarchy with a level 1 beyond k_resident's 2048 rows (the Newton systems of the m = n = 2048
// runs): candidate for the mask-form kernel's DEEP mode (ipd_resident_big.h) -- it needs the bit mask
// whatever the population of the rows
inline bool resident_deep_candidate(const ResidentInputs& in, const PlanSwitches& sw, const ResidentFacts& f) {
    const ImageRole img = resident_deep_image(in);
    return !sw.no_resident && !sw.no_resident_big && !sw.no_resident_deep && !f.off && !f.ok && !f.mask_form &&
           !in.small_ok && !in.twogrid && in.cyc() && in.smoth >= 1 && in.J >= 5 &&
           (f.n + f.m > RES_NMAX || sw.resident_big) && in.L[1].nf == f.n && in.L[1].nr == f.m + f.n &&
           resident_deep_sizes_fit(f.n, f.m, in.L[2].nr, in.L[3].nr, in.L[4].nr) && img != IMG_NONE &&
           std::max(RB_LDS_BYTES, in.img[img].lds) <= RES_LDS_MAX;
}

// DEEP mode of the mask-form kernel: realistic hierarchies (five levels and more) whose level 1 exceeds
// k_resident's 2048 rows.  Level 2 as short register slices, level 3 in polynomial form (pack_bpoly in the
// RB_P3_SEG row layout), the LDS image rooted at level 4 for the tail workgroup; G <= 255 workgroups
// (the tail needs a compute unit of its own), two rows of each block per wave.
inline ResidentPlan plan_resident_deep(const ResidentInputs& in, const PlanSwitches& sw, const ResidentFacts& f) {
    ResidentPlan p;
    if (!resident_deep_candidate(in, sw, f)) return p;
    const int n = f.n, m = f.m, N3 = in.L[3].nr, N4 = in.L[4].nr;
    int G = std::max(std::max(resident_cdiv(std::max(n, m), 2 * RES_WAVES), resident_cdiv(N3, 4)), std::max(N4, 128));
    G = std::max(G, sw.resident_g);
    p.S[2] = resident_stride(in, 2, &p.priv[2]);
    // level 4 resident as well (POLY4), the tail rooted at level 5: the only form an image rooted at level 5 serves
    const int N5 = in.J >= 6 ? in.L[5].nr : 0;
    const bool poly4 = in.have5() && in.k_sub == 5 && N4 <= 2 * G && N5 >= 1 && N5 <= G && N5 <= RB_N5MAX &&
                       N4 + G <= BT && std::max(RB_LDS_BYTES, in.img[in.sub5].lds) <= RES_LDS_MAX;
    if (!(G + 1 <= in.num_cu && G <= std::min(n, m) && p.S[2] > 0 && p.S[2] <= 64 * 8 && (poly4 || in.k_sub != 5)))
        return p;
    p.kind = RESIDENT_DEEP;
    p.key = ResidentKey::mask(p.S[2] <= 64 * 4 ? 4 : 8, 2, true);
    p.G = G;
    p.remote = true;
    p.poly3 = true;
    p.poly4 = poly4;
    p.tail_root = poly4 ? 5 : 4;
    p.tail_image = poly4 ? in.sub5 : resident_deep_image(in);
    p.lds = std::max(RB_LDS_BYTES, in.img[p.tail_image].lds);
    p.levels = poly4 ? 4 : 3;
    return p;
}
