// Level planner of the single-workgroup kernels: from the level sizes and the options alone it decides
// each level's form (polynomial, block-wide polynomial, dense thread-per-row, thread-per-row, tiny
// dense) and which LDS images are packed -- the whole solve, the sub-cycle and the images rooted at
// levels 3 and 4 the resident kernels take -- with their LDS budget.  amg_prepare_levels packs what it
// returns (pack_image, ipd_image.hip).  What an image holds -- its pieces, their sizes and LDS offsets
// -- is written down here once (image_layout): plan_lds sums the pieces to decide what fits, pack_image
// binds them to the descriptor.  Host-clean, no HIP: tests/level_plan_driver.cpp runs it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <numeric>
#include <vector>

#include "ipd_launch_plan.h"
#include "ipd_limits.h"

struct LevelShape {   // level k of the hierarchy, as far as the planner looks at it
    int nr = 0;       // rows
    int nnz = 0;      // entries of A_k
    int nf = 0;       // F-block size (level 1 of a bigraph hierarchy; 0 = Jacobi)
    int maxoff = 0;   // longest off-diagonal row (0 where the level's data come from a donor)
    int p_nnz = 0;    // entries of P_k (level k-1 <- k), k >= 2
};

struct PlanOptions {
    char cycle = 'v';
    int smoth = 1;
    bool twogrid = false, concurrent_pair = false;
    size_t sol_head = SOL_HEAD;   // the image head (SolveDesc and its relocation table)
};

// The switches of the launch planner (ipd_launch_plan.h), of the level planner and of the resident planner
// (ipd_switches.h), read by read_plan_switches at the call in which they take effect: amg_prepare_levels and
// again amg_attach_maskop
struct PlanSwitches : LaunchSwitches {
    bool no_poly = false, no_blk = false, no_bpoly = false, no_blkdense = false, no_small = false,
         no_subcycle = false, no_resident = false, no_resident_remote = false, no_resident_three = false,
         no_resident_deep = false, no_resident_big = false, no_res_poly4 = false;
    bool resident_big = false, maskop = false;   // IPD_RESIDENT_BIG, IPD_MASKOP
    int resident_g = 0, resident_ranks = 0;      // IPD_RESIDENT_G, IPD_RESIDENT_RANKS (0: unset)
    int res_presleep = -1;                       // IPD_RES_PRESLEEP (-1: unset)
    unsigned res_skip_publish = 0;               // IPD_RES_DEBUG_SKIP_PUBLISH
    bool res_no_full = false;                    // IPD_RES_NO_FULL: k_resident's general form where the full-shape one applies
};

enum ImageRole { IMG_SOLVE, IMG_SUB, IMG_SUB3, IMG_SUB4, IMG_NONE };

struct ImageSpec {
    ImageRole role;
    int k_lds;            // first level of the image (its root; > J: the whole solve with nothing cached)
    int k_semi;           // semi-cached root level (vectors in LDS, rows from L2), 0 = none
    int k_tiny;           // first tiny (dense) level
    int k_blk;            // first thread-per-row level (J + 1: none, the generic phases)
    size_t stage_bytes;   // staging area in front of the image
    size_t lds;           // predicted dynamic LDS (plan_lds)
    int k_cached;         // the first level that plan_lds run cached (<= k_lds; k_semi + 1 under a semi-cached root)
};

static inline size_t plan_r8(size_t n) { return (n + 7) / 8 * 8; }
static inline size_t plan_r16(size_t b) { return (b + 15) / 16 * 16; }
static inline size_t poly_ld(size_t rows) { return rows <= 32 ? 32 : (rows <= 48 ? 48 : 64); }
static inline int bpoly_ld(int N, int Nc) { return N + Nc <= 128 ? 128 : 256; }
static inline size_t bp_part_bytes(size_t LD) { return 8 * (8 * LD + 8); }   // partial sums of a block-wide polynomial pass

// ---- What an image is made of ---------------------------------------------------------------------------
// The form of a level in an image: semi-cached root (vectors only), CSR arrays (thread-per-row, or the
// generic phases), dense thread-per-row copy, tiny dense, one-wave polynomial, block-wide polynomial out
// of LDS, block-wide polynomial with the operators in L2
enum LevelForm { FORM_SEMI, FORM_CSR, FORM_BDENSE, FORM_TINY, FORM_POLY, FORM_LPOLY, FORM_BPOLY };
static inline bool block_wide(LevelForm f) { return f == FORM_LPOLY || f == FORM_BPOLY; }
static inline bool polynomial(LevelForm f) { return f == FORM_POLY || block_wide(f); }
static inline LevelForm level_form(const ImageSpec& s, int k, bool poly, bool lpoly, bool bpoly, bool bdense) {
    if (k == s.k_semi) return FORM_SEMI;
    const bool tiny = k >= s.k_tiny;
    if (s.k_blk <= k) {
        if (tiny ? poly : lpoly) return tiny ? FORM_POLY : FORM_LPOLY;
        if (!tiny && bpoly) return FORM_BPOLY;
        if (!tiny && bdense) return FORM_BDENSE;
    }
    return tiny ? FORM_TINY : FORM_CSR;
}

// The pointers of the descriptor (SolveDesc) that point into LDS, in the order of the image
enum ImageSlot {
    SLOT_RP, SLOT_CI, SLOT_VA, SLOT_DINV, SLOT_AXI, SLOT_XX,                              // the level's constants
    SLOT_REST_RP, SLOT_REST_CI, SLOT_REST_VA, SLOT_PROL_RP, SLOT_PROL_CI, SLOT_PROL_VA,   // transfers to level k + 1
    SLOT_LMAP, SLOT_DA, SLOT_DP, SLOT_DPT, SLOT_PMR, SLOT_PME, SLOT_PMC, SLOT_PW,         // blocks computed into the image
    SLOT_R, SLOT_E, SLOT_E2, SLOT_RR, SLOT_W,                                             // work vectors
    SLOT_BP_PART, SLOT_PCG_WORK,                                                          // work areas: image-wide, coarsest level
    SLOT_REST_X, SLOT_REST_Y, SLOT_PCG_RP, SLOT_PCG_CI, SLOT_PCG_VA,                      // always aliases
    SLOT_COUNT
};
// how a piece gets its content: copied from global memory, computed by k_pack_dense / k_pack_lmap /
// k_pack_poly, a work vector (zeroed on arrival), or the address of another piece
enum PieceKind { PIECE_COPY, PIECE_DENSE, PIECE_LMAP, PIECE_POLY, PIECE_WORK, PIECE_ALIAS };
static inline PieceKind slot_kind(ImageSlot s) {
    return s <= SLOT_PROL_VA ? PIECE_COPY : s == SLOT_LMAP ? PIECE_LMAP : s <= SLOT_DPT ? PIECE_DENSE : s <= SLOT_PW ? PIECE_POLY : PIECE_WORK;
}

// which slots a level of a given form owns (transfers: above the coarsest level only; lane map: see has)
static constexpr unsigned slot_bits(int first, int last) { return ((2u << last) - 1u) & ~((1u << first) - 1u); }
static constexpr unsigned SLOTS_VECTORS = slot_bits(SLOT_R, SLOT_W), SLOTS_XFER = slot_bits(SLOT_REST_RP, SLOT_PROL_VA),
                          SLOTS_ROWS = slot_bits(SLOT_RP, SLOT_RP) | slot_bits(SLOT_DINV, SLOT_XX) | SLOTS_XFER | SLOTS_VECTORS;
static constexpr unsigned FORM_SLOTS[] = {
    /* FORM_SEMI   */ SLOTS_VECTORS,
    /* FORM_CSR    */ SLOTS_ROWS | slot_bits(SLOT_CI, SLOT_VA) | slot_bits(SLOT_LMAP, SLOT_LMAP),
    /* FORM_BDENSE */ SLOTS_ROWS | slot_bits(SLOT_DA, SLOT_DA),
    /* FORM_TINY   */ SLOTS_ROWS | slot_bits(SLOT_CI, SLOT_VA) | slot_bits(SLOT_DA, SLOT_DPT),
    /* FORM_POLY   */ slot_bits(SLOT_XX, SLOT_XX) | slot_bits(SLOT_PMR, SLOT_PW) | SLOTS_VECTORS,
    /* FORM_LPOLY  */ slot_bits(SLOT_XX, SLOT_XX) | slot_bits(SLOT_PMR, SLOT_PW) | SLOTS_VECTORS,
    /* FORM_BPOLY  */ slot_bits(SLOT_XX, SLOT_XX) | SLOTS_VECTORS};

// Level k of an image in a given form: which pieces it owns and how large they are
struct LevelPieces {
    const LevelShape* L;
    int J, k;
    LevelForm form;
    bool lean;      // rr and w are never dereferenced: aliases of e2 (see choose_forms)
    bool lmap_ok;   // a thread-per-row level that takes a lane map (unless it is the coarsest)
    bool pad8;      // vectors zero-padded to whole 8-entry blocks (one-wave levels: sol_load_image; polynomial
                    // levels and the children of block-wide ones: bpoly_pass)

    size_t ld() const {   // leading dimension of the level's polynomial operators
        return form == FORM_POLY    ? poly_ld((size_t)L[k].nr + (size_t)L[k + 1].nr)
               : form == FORM_LPOLY ? 64
                                    : (size_t)bpoly_ld(L[k].nr, L[k + 1].nr);
    }
    // (dense thread-per-row levels: whole groups of four entries per lane, dense_row_dot)
    size_t vec_len() const {
        return form == FORM_BDENSE ? (size_t)bdense_pad(L[k].nr) : pad8 ? plan_r8((size_t)L[k].nr) : (size_t)L[k].nr;
    }
    bool has(ImageSlot s) const {
        if (s == SLOT_PCG_WORK) return k == J;
        if (s > SLOT_W || !(FORM_SLOTS[form] >> s & 1u)) return false;
        if (s == SLOT_LMAP) return lmap_ok && k < J;
        return k < J || !((SLOTS_XFER | slot_bits(SLOT_DP, SLOT_DPT)) >> s & 1u);
    }
    bool alias(ImageSlot s) const { return lean && (s == SLOT_RR || s == SLOT_W); }
    size_t bytes(ImageSlot s) const {
        const size_t N = (size_t)L[k].nr, nnz = (size_t)L[k].nnz, Nc = k < J ? (size_t)L[k + 1].nr : 0,
                     np = k < J ? (size_t)L[k + 1].p_nnz : 0, LD = polynomial(form) ? ld() : 0, v = 8 * vec_len();
        const size_t in_slot_order[] = {
            4 * (N + 1), 4 * nnz, 8 * nnz, 8 * N, 8 * N, 8,                                         // rp ci va dinv Axi xx
            4 * (Nc + 1), 4 * np, 8 * np, 4 * (N + 1), 4 * np, 8 * np,                              // rest, prol: rp ci va
            4 * ((size_t)BT + 1), form == FORM_BDENSE ? 8 * N * (size_t)bdense_ld((int)N) : 8 * N * N, 8 * N * Nc, 8 * N * Nc,   // lmap dA dP dPt
            8 * LD * plan_r8(N), 8 * LD * plan_r8(N), 8 * LD * plan_r8(Nc), 8 * LD,                 // pMr pMe pMc pW
            v, v, v, v, v, 0, 4 * N * 8};                                                           // r e e2 rr w, -, pcg.work
        return s <= SLOT_PCG_WORK ? in_slot_order[s] : 0;
    }
    size_t sum() const {   // LDS the level's own pieces take
        size_t b = 0;
        for (int s = SLOT_RP; s <= SLOT_PCG_WORK; ++s)
            if (has((ImageSlot)s) && !alias((ImageSlot)s)) b += plan_r16(bytes((ImageSlot)s));
        return b;
    }
};
static inline LevelPieces level_pieces(const LevelShape* L, int J, const ImageSpec& s, bool lean_vectors, int k,
                                       LevelForm form, bool below_block_wide) {
    LevelPieces p{L, J, k, form, false, false, false};
    p.lean = lean_vectors && s.k_blk <= std::max(2, s.k_lds) && k >= 2;
    p.lmap_ok = lean_vectors && form == FORM_CSR && s.k_blk <= k && k >= 2 && L[k].nr <= BT;
    p.pad8 = k >= s.k_tiny || polynomial(form) || below_block_wide;
    return p;
}

// What plan_lds counts on top of the pieces.  Every term is an over-count, kept because it decides which
// levels are admitted near the budget: dropping one changes plans.
static constexpr size_t RESERVE_HEAD = 256;           // once per image; nothing is carved for it
static constexpr size_t RESERVE_XX_POLY = 16;         // a polynomial level's 16-byte xx slot is counted as 32 B ...
static constexpr size_t RESERVE_XX_BPOLY = 32;        // ... and as 48 B where the operators stay in L2
static constexpr size_t RESERVE_CHILD_PAD = 5 * 64;   // bounds the padding of the vectors of a level below a block-wide polynomial
                                                      // one (carved: at most 3 x 48 B, none under a parent outside the image)
enum Reserve {
    RSV_HEAD, RSV_XX,
    RSV_BP_PART,         // bp_part is counted for every block-wide polynomial level, carved once at the largest LD
    RSV_CHILD_PAD,
    RSV_COARSEST_LMAP,   // the lane map is counted for a thread-per-row coarsest level, which gets none
    RSV_CONST_PAD,       // dinv and Axi are counted at the padded length of the level's work vectors
    RSV_ABOVE_ROOT,      // levels the plan_lds run cached above the root of the image (ImageSpec::k_cached)
    RSV_COUNT
};
struct ImageReserves {
    size_t of[RSV_COUNT] = {};
    size_t sum() const { return std::accumulate(of, of + RSV_COUNT, (size_t)0); }
};
// level k as plan_lds counts it -- deepest first, before the image it ends up in is known: as the root of an
// image of its own
static inline ImageSpec level_alone(int k, int tiny_lo) {
    return ImageSpec{IMG_NONE, k, 0, std::max(tiny_lo, std::max(2, k)), std::max(2, k), 0, 0, k};
}
static inline ImageReserves level_reserves(const LevelPieces& p, bool below_block_wide) {
    ImageReserves r;
    if (polynomial(p.form)) r.of[RSV_XX] = p.form == FORM_BPOLY ? RESERVE_XX_BPOLY : RESERVE_XX_POLY;
    if (block_wide(p.form)) r.of[RSV_BP_PART] = plan_r16(bp_part_bytes(p.ld()));
    if (!polynomial(p.form)) {
        r.of[RSV_CONST_PAD] = 2 * (plan_r16(8 * p.vec_len()) - plan_r16(8 * (size_t)p.L[p.k].nr));
        if (below_block_wide) r.of[RSV_CHILD_PAD] = RESERVE_CHILD_PAD;
        if (p.lmap_ok && p.k == p.J) r.of[RSV_COARSEST_LMAP] = plan_r16(p.bytes(SLOT_LMAP));
    }
    return r;
}

struct ImagePiece {
    int level;   // 0: image-wide
    ImageSlot slot;
    PieceKind kind;
    size_t bytes;   // as copied or computed; the next piece starts plan_r16(bytes) further on
    size_t off;     // LDS offset from the start of dynamic LDS (the staging area included); PIECE_ALIAS: of the other piece
};
struct ImageLayout {
    std::vector<ImagePiece> pieces;   // in the order of the image; each is one relocation of the descriptor
    size_t image_bytes = 0;           // head, constants and computed blocks: what is copied to LDS behind the staging area
    size_t total = 0;                 // dynamic LDS of a launch: staging area, image, work vectors
    const ImagePiece* find(int level, ImageSlot slot) const {
        for (const ImagePiece& p : pieces)
            if (p.level == level && p.slot == slot) return &p;
        return nullptr;
    }
};

struct LevelPlan {
    int J = 0;
    bool use_poly = false, use_lpoly = false, lean_vectors = false;
    int tiny_lo = 0;
    // per level (index 1..J): polynomial forms of the one-wave (poly) and block-wide (lpoly: out of LDS,
    // bpoly: operators in global memory) kinds, dense thread-per-row copy
    std::vector<char> poly, lpoly, bpoly, bdense;
    std::vector<ImageSpec> images;   // in packing order
    bool small_ok = false;           // an IMG_SOLVE image is planned
    int k_sub = 0;                   // root of the IMG_SUB image, 0 = none
    bool sub_semi_root = false;
    ImageRole sub5 = IMG_NONE;       // the image that serves the tail rooted at level 5 (d_sub5)

    const ImageSpec* image(ImageRole r) const {
        for (const ImageSpec& s : images)
            if (s.role == r) return &s;
        return nullptr;
    }
    LevelForm form(const ImageSpec& s, int k) const {
        return level_form(s, k, poly[(size_t)k], lpoly[(size_t)k], bpoly[(size_t)k], bdense[(size_t)k]);
    }
    LevelPieces pieces(const LevelShape* L, const ImageSpec& s, int k) const {
        return level_pieces(L, J, s, lean_vectors, k, form(s, k), k > s.k_lds && block_wide(form(s, k - 1)));
    }
    // level k of image s is a thread-per-row level (BT threads dealt to its rows)
    bool thread_per_row(const ImageSpec& s, int k) const {
        return k >= std::max(s.k_lds, s.k_blk) && k <= J && (form(s, k) == FORM_CSR || form(s, k) == FORM_BDENSE);
    }
};

// The image of spec s, piece by piece: the constants of levels k_lds..J, lane maps, dense thread-per-row
// copies, block-wide polynomial operators, one-wave polynomial or tiny dense blocks; behind the image the
// work vectors, bp_part and the coarsest PCG's work area.  (s.k_lds <= J: a solve with nothing cached has none.)
inline ImageLayout image_layout(const LevelShape* L, const LevelPlan& plan, const ImageSpec& s) {
    constexpr unsigned ANY_FORM = ~0u;
    ImageLayout lay;
    const int J = plan.J;
    size_t off = s.stage_bytes + SOL_HEAD;
    auto place = [&](int k, ImageSlot slot, PieceKind kind, size_t bytes) {
        lay.pieces.push_back(ImagePiece{k, slot, kind, bytes, off});
        off += plan_r16(bytes);
    };
    auto alias = [&](int k, ImageSlot slot, int of_level, ImageSlot of_slot) {
        lay.pieces.push_back(ImagePiece{k, slot, PIECE_ALIAS, 0, lay.find(of_level, of_slot)->off});
    };
    auto pass = [&](ImageSlot first, ImageSlot last, unsigned forms) {
        for (int k = s.k_lds; k <= J; ++k) {
            const LevelPieces p = plan.pieces(L, s, k);
            if (!(forms >> p.form & 1u)) continue;
            for (int q = first; q <= last; ++q) {
                const ImageSlot slot = (ImageSlot)q;
                if (!p.has(slot)) continue;
                p.alias(slot) ? alias(k, slot, k, SLOT_E2) : place(k, slot, slot_kind(slot), p.bytes(slot));
            }
        }
    };
    pass(SLOT_RP, SLOT_PROL_VA, ANY_FORM);
    pass(SLOT_LMAP, SLOT_LMAP, ANY_FORM);
    pass(SLOT_DA, SLOT_DA, 1u << FORM_BDENSE);
    pass(SLOT_PMR, SLOT_PW, 1u << FORM_LPOLY);
    pass(SLOT_DA, SLOT_PW, 1u << FORM_TINY | 1u << FORM_POLY);
    lay.image_bytes = off - s.stage_bytes;
    pass(SLOT_R, SLOT_W, ANY_FORM);
    size_t bp_ld = 0;
    for (int k = s.k_lds; k < J; ++k)
        if (block_wide(plan.form(s, k))) bp_ld = std::max(bp_ld, plan.pieces(L, s, k).ld());
    if (bp_ld) place(0, SLOT_BP_PART, PIECE_WORK, bp_part_bytes(bp_ld));
    for (int k = std::max(1, s.k_lds - 1); k < J; ++k) {   // vectors that cross levels
        if (k >= s.k_lds) alias(k, SLOT_REST_X, k, SLOT_RR);
        alias(k, SLOT_REST_Y, k + 1, SLOT_R);
    }
    for (int q = 0; q < 3; ++q) alias(0, (ImageSlot)(SLOT_PCG_RP + q), J, (ImageSlot)(SLOT_RP + q));   // the coarsest PCG's CSR arrays
    pass(SLOT_PCG_WORK, SLOT_PCG_WORK, ANY_FORM);
    lay.total = off;
    return lay;
}

// Conditions of the resident planner (ipd_resident_plan.h) that this one anticipates when it packs images for it
// workgroups of k_resident: one wave per row of the larger block of level 1 and of level 2
static inline int resident_rows_G(int nf, int nc, int N2) {
    return std::max((std::max(nf, nc) + RES_WAVES - 1) / RES_WAVES, (N2 + RES_WAVES - 1) / RES_WAVES);
}
// k_resident's POLY3: the tail's root level 4 has one restriction row per workgroup at most
static inline bool resident_poly3_root_fits(int N4, int G) { return N4 <= G && N4 <= 128; }
// the mask-form kernel's deep mode: blocks of level 1 (nf, nc), level 2 = the C block, levels 3 and 4
static inline bool resident_deep_sizes_fit(int nf, int nc, int N2, int N3, int N4) {
    return nf <= RB_HALF && nc <= RB_HALF && N2 == nc && N3 <= RB_N3MAX && N4 <= RB_N4MAX;
}

struct LevelPlanner {
    const LevelShape* L;   // 1..J
    int J;
    PlanOptions o;
    PlanSwitches sw;
    bool cyc;
    // decided on the way (see plan_levels)
    bool use_poly, use_lpoly, lean_vectors, use_lmap, use_bdense, use_bpoly;
    int tiny_lo;

    // one workgroup is one CU: beyond ~1000 short rows per level the multi-launch path (many CUs per
    // phase) wins again (measured: M = 1000 W-cycle solve 9.5 ms here vs 17 ms multi-launch; M = 2048:
    // 8.0 ms here vs 5.6 ms multi-launch).  The transfer to a level at or above k_root is not looked at.
    bool small_level(int k, int k_root = 1) const {
        return L[k].nr <= 1024 && L[k].nnz <= 40000 && (k <= k_root || L[k].p_nnz <= 40000);
    }
    // bottom run of levels with <= 32 rows (k >= 2): candidates for the wave-level sub-cycle
    // (33..64 rows run faster block-wide with 16 lanes per row than in one wave) -- <= 48 rows when
    // the one-wave levels take the polynomial form (tiny_cycle: a visit is two dense passes whatever
    // the row count; IPD_NO_POLY=1: sweeps)
    int find_tiny_lo(int rows_max) const {
        int lo = J + 1;
        for (int k = J; k >= 2; --k) {
            if (L[k].nr > rows_max) break;
            if (rows_max > 32 && use_lpoly && k < J && L[k].nr + L[k + 1].nr > 32) break;
            lo = k;
        }
        return lo;
    }
    bool is_poly(int k) const { return use_poly && k >= tiny_lo && k < J && L[k].nr + L[k + 1].nr <= 64; }
    // (polynomial form: a level whose stacked operator [e'; r_c] has more than 32 rows -- one lane per row in
    // a single wave -- runs block-wide instead, out of LDS all the same)
    bool is_lpoly(int k) const {
        return use_poly && use_lpoly && lean_vectors && k >= 2 && k < tiny_lo && k < J && L[k].nr <= 48 &&
               L[k].nr + L[k + 1].nr <= 64;
    }
    // thread-per-row levels of 33..144 rows in block-wide polynomial form (SolveLevel::gM)
    bool is_bpoly(int k) const {
        if (!use_poly || !use_bpoly || k < 2 || k >= J || k >= tiny_lo) return false;
        const long long N = L[k].nr, Nc = L[k + 1].nr;
        // (up to 224 rows below a level 1 of more than 2048 rows: there level 4 has 150-200 rows, often dense --
        // 23 k entries do not fit an LDS image, the operators of this form stay in L2 -- and the mask-form
        // resident kernel needs its tail rooted at level 4, ipd_resident_big.h DEEP)
        const long long nmax = L[1].nr > RES_NMAX ? 224 : 144;
        return N > 32 && N <= nmax && N + Nc <= 256 && 2 * ((N + 7) / 8 * 8) + (Nc + 7) / 8 * 8 <= 512 && !is_lpoly(k);
    }
    // small, nearly full thread-per-row levels: dense copy instead of the CSR arrays (see SolveLevel::blk_dense)
    bool is_bdense(int k) const {
        if (!use_bdense || k < 2 || k >= J || k >= tiny_lo || is_bpoly(k)) return false;
        const long long N = L[k].nr;
        return N > 32 && N <= 96 && bdense_pad((int)N) / bdense_lanes((int)N) <= BDENSE_Q && 3LL * L[k].nnz >= N * N;
    }
    // level k as plan_lds counts it (level_alone): its form there
    LevelForm form_alone(int k) const {
        return level_form(level_alone(k, tiny_lo), k, is_poly(k), is_lpoly(k), is_bpoly(k), is_bdense(k));
    }
    // LDS cache plan: deepest levels first, while they fit; returns the first cached level.  A level counts
    // with its pieces in its form (LevelPieces) and the reserves named above.
    int plan_lds(size_t stage, size_t* used_out) const {
        size_t used = stage + o.sol_head + RESERVE_HEAD;
        int k_lds = J + 1;
        for (int k = J; k >= 1; --k) {
            const LevelPieces p = level_pieces(L, J, level_alone(k, tiny_lo), lean_vectors, k, form_alone(k), false);
            // (the thread-per-row sub-cycle deals BT threads to the rows: a level of more than BT rows cannot
            // be held that way -- it fits the budget once its child's operators stay in L2, block-wide
            // polynomial form of a 150-224-row level 4 below a 576-row level 3)
            if (!polynomial(p.form) && k >= 2 && L[k].nr > BT) break;
            const size_t bytes = p.sum() + level_reserves(p, k >= 2 && block_wide(form_alone(k - 1))).sum();
            if (used + bytes > IMAGE_LDS_BUDGET) break;
            used += bytes;
            k_lds = k;
        }
        *used_out = used;
        return k_lds;
    }
    int tiny_from(int k_lds) const { return std::max(tiny_lo, std::max(2, k_lds)); }   // tiny levels: cached, Jacobi (k >= 2)
    int blk_from(int k_lds) const { return (sw.no_blk || k_lds > J) ? J + 1 : std::max(2, k_lds); }   // thread-per-row levels
    // Level 2 as a semi-cached level (r, e, e2 in LDS; matrix rows from L2) with levels 3..J fully
    // cached: returns the dynamic LDS needed behind a staging area of `stage` bytes, 0 = no
    size_t semi_plan(size_t stage) const {
        if (!lean_vectors || J < 3 || J > SOLVE_ML) return 0;
        if (L[2].nr > BT || L[2].nr <= 64 || (double)L[2].nnz > 12.0 * L[2].nr || (double)L[3].p_nnz > 12.0 * L[2].nr)
            return 0;
        for (int k = 3; k <= J; ++k)
            if (!small_level(k)) return 0;
        size_t used = 0;
        const int k_lds = plan_lds(stage, &used);
        if (k_lds != 3) return 0;   // <= 2: level 2 fits entirely; > 3: a deeper level does not
        const size_t need = used + 3 * plan_r16(8 * (size_t)L[2].nr);
        return need <= IMAGE_LDS_BUDGET ? need : 0;
    }
    // an image rooted at level k (the sub-cycle and the resident kernels' tails)
    ImageSpec rooted(ImageRole role, int k, bool semi, size_t stage, size_t lds, int k_cached) const {
        return ImageSpec{role, k, semi ? k : 0, tiny_from(k + (semi ? 1 : 0)), blk_from(k), stage, lds, k_cached};
    }

    void choose_forms();
    void plan_solve(LevelPlan& p) const;
    void plan_sub(LevelPlan& p) const;
    void plan_tails(LevelPlan& p) const;
};

// The levels' forms: the polynomial forms are taken, but not at the price of a level that would
// otherwise be cached.
inline void LevelPlanner::choose_forms() {
    use_poly = o.smoth >= 1 && cyc && !sw.no_poly && !sw.no_blk;
    use_lpoly = !sw.no_blk;
    tiny_lo = find_tiny_lo(use_poly ? 48 : 32);
    // the thread-per-row / wave sub-cycles keep the residual in the free iterate buffer and never
    // use the Gauss-Seidel scratch vector: 5 vectors per cached level instead of 7
    lean_vectors = !sw.no_blk;
    use_lmap = lean_vectors;
    use_bdense = lean_vectors && !sw.no_blkdense;
    use_bpoly = lean_vectors && !sw.no_bpoly;
    if (!use_poly) return;
    size_t u = 0;
    const int with_poly = plan_lds(16, &u);
    const int lo_poly = tiny_lo;
    use_poly = false;
    tiny_lo = find_tiny_lo(32);
    const int without = plan_lds(16, &u);
    if (with_poly <= without) {
        use_poly = true;
        tiny_lo = lo_poly;
    } else if (use_lpoly) {
        // the block-wide form out of LDS pads its operators to 64 rows: where that is what does not
        // fit, the one-wave form (48 rows) may still
        use_lpoly = false;
        use_poly = true;
        tiny_lo = find_tiny_lo(48);
        if (plan_lds(16, &u) > without) {
            use_poly = false;
            tiny_lo = find_tiny_lo(32);
        }
    }
}

// (a) the whole solve in one workgroup when every level is small
inline void LevelPlanner::plan_solve(LevelPlan& p) const {
    bool ok = !sw.no_small && J <= SOLVE_ML;
    size_t maxlen = 1;
    for (int k = 1; k <= J && ok; ++k) {
        ok = ok && small_level(k);
        maxlen = std::max(maxlen, (size_t)L[k].nr);
    }
    if (!ok) return;
    const size_t stage = plan_r16(sizeof(double) * maxlen);
    size_t used = 0;
    const int k_lds = plan_lds(stage, &used);
    p.images.push_back(ImageSpec{IMG_SOLVE, k_lds, 0, tiny_from(k_lds), blk_from(k_lds), stage, used, k_lds});
    p.small_ok = true;
}

// (b) otherwise the sub-cycle below the first level from which everything fits in LDS runs as one
// launch per visit
inline void LevelPlanner::plan_sub(LevelPlan& p) const {
    if (sw.no_subcycle || p.small_ok || J > SOLVE_ML || J < 3 || !cyc) return;
    if (const size_t need = semi_plan(16)) {   // (b1) the sub-cycle is rooted at the semi-cached level 2
        p.images.push_back(rooted(IMG_SUB, 2, true, 16, need, 3));
        p.k_sub = 2;
        return;
    }
    // first level from which every level is small ...
    int k_small = J + 1;
    for (int k = J; k >= 2 && small_level(k); --k) k_small = k;
    // Level 1 of 2049..4096 rows, six levels or more: the mask-form resident kernel's deep mode keeps
    // levels 3 AND 4 in polynomial form in its workgroups and roots its tail workgroup at level 5
    // (ipd_resident_big.h, POLY4) -- ONE image, rooted at level 5, serves it and the launches (which
    // then run level 4 as launches: the fall-back).  (An image rooted at level 4 for the launches
    // beside one rooted at level 5 for the resident kernel packed levels 5..J twice: 0.2 ms per hierarchy.)
    const int nf1 = L[1].nf, nc1 = L[1].nr - nf1;
    const bool root5 = J >= 6 && L[1].nr > RES_NMAX && nf1 > 0 &&
                       resident_deep_sizes_fit(nf1, nc1, L[2].nr, L[3].nr, L[4].nr) && L[5].nr <= RB_N5MAX && o.smoth >= 1 && !o.twogrid &&
                       !o.concurrent_pair && !sw.no_res_poly4 && !sw.no_resident_deep && !sw.no_resident_big &&
                       !sw.no_resident;
    if (root5) k_small = std::max(k_small, 5);
    // ... and everything below it fits in LDS
    for (int kroot = k_small; kroot < J; ++kroot) {
        // the generic phases (and their staging vector of N_root doubles) only run when IPD_NO_BLK is set
        const size_t stage = lean_vectors ? 16 : plan_r16(sizeof(double) * (size_t)L[kroot].nr);
        size_t used = 0;
        const int k_lds = plan_lds(stage, &used);
        // the root itself does not fit beside the deeper levels but has at most BT rows (a
        // level 3 of 170-310 rows with 40-100 entries each in the m=n=1024 runs): it becomes a
        // semi-cached root -- vectors in LDS, rows walked from L2 by several lanes each
        // (glb_rowdot_range), 2-3 us per sweep against 5 us for the launch it replaces
        // (only with short rows, <= 12 entries on average like the semi-cached level 2: measured on
        // the Newton systems of the m=n=1024 Class 1 run, a level 3 of 2-3 k entries gains 5-9 % per W
        // cycle as launches and opens the hierarchy to the resident kernel's remote tail, -15...-23 %;
        // with 4 k entries it loses 12 %, with 9-17 k entries a sweep from L2 through one CU costs
        // more than the launch: 0.72 -> 1.09 ms, 0.54 -> 1.21 ms per W cycle)
        const size_t semi_need = used + 3 * plan_r16(8 * (size_t)L[kroot].nr);
        const bool semi_root = k_lds == kroot + 1 && kroot >= 3 && lean_vectors && L[kroot].nr <= BT &&
                               (double)L[kroot].nnz <= 12.0 * L[kroot].nr &&
                               (double)L[kroot + 1].p_nnz <= 12.0 * L[kroot].nr && semi_need <= IMAGE_LDS_BUDGET;
        if (k_lds > kroot && !semi_root) continue;
        p.images.push_back(rooted(IMG_SUB, kroot, semi_root, stage, semi_root ? semi_need : used, k_lds));
        p.k_sub = kroot;
        p.sub_semi_root = semi_root;
        return;
    }
}

// Images for the resident kernels' tail workgroups alone, and the image that serves a tail rooted at level 5
inline void LevelPlanner::plan_tails(LevelPlan& p) const {
    size_t used = 0;
    // (b2) Where level 3 is only a semi-cached root (its rows come from L2), the level-resident kernel
    // does better with level 3 in registers and its tail rooted at level 4 (plan_resident, `three`:
    // 0.50-0.51 against 0.57-0.61 ms per W cycle on the Newton systems of the m=n=1024 Class 1 run), so a
    // second image rooted at level 4 is packed for it.  (Where levels 3..J fit the image as they are,
    // the tail rooted at level 3 stays 3-6 % ahead: 0.49-0.51 against 0.51-0.54 ms.)
    // With level 3 in polynomial form (plan_resident, poly3: a visit of it is three hand-offs instead of
    // thirteen) the same holds wherever that form applies, semi-cached root or not: 0.33-0.36 -> see DESIGN.
    const bool poly3_likely =
        J >= 5 && o.smoth >= 1 && L[1].nf > 0 &&
        resident_poly3_root_fits(L[4].nr, resident_rows_G(L[1].nf, L[1].nr - L[1].nf, L[2].nr)) && !sw.no_poly;
    if (p.k_sub == 3 && (p.sub_semi_root || poly3_likely) && J >= 5 && J <= SOLVE_ML && L[3].nr <= BT &&
        L[4].nr <= BT && L[3].maxoff <= 512 && L[1].nf > 0 && !sw.no_resident_three && !sw.no_resident) {
        bool ok = lean_vectors;
        for (int k = 4; k <= J && ok; ++k) ok = small_level(k);
        const int k_lds = ok ? plan_lds(16, &used) : J + 1;
        if (k_lds <= 4) p.images.push_back(rooted(IMG_SUB4, 4, false, 16, used, k_lds));
    }
    // (b3) No sub-cycle at all because level 3's interpolation is big (P_3 with more than 40 k entries:
    // a dense 1024 x 50 block early in a run), although levels 3..J themselves are small: the launch
    // path would gain nothing from an image whose restriction and prolongation stay launches, but the
    // resident kernel's remote tail does not use P_3 from the image -- its workgroups apply it -- so an
    // image rooted at level 3 is packed for it alone.
    if (p.k_sub == 0 && !p.small_ok && J >= 4 && J <= SOLVE_ML && lean_vectors && L[3].nr <= BT && L[1].nf > 0 &&
        cyc && !sw.no_resident && !sw.no_subcycle) {
        bool ok = true;
        for (int k = 3; k <= J && ok; ++k) ok = small_level(k, 3);
        const int k_lds = ok ? plan_lds(16, &used) : J + 1;
        if (k_lds <= 3) p.images.push_back(rooted(IMG_SUB3, 3, false, 16, used, k_lds));
    }
    // (b4) the image rooted at level 5 (see root5, plan_sub) is the one the deep mode's tail workgroup takes
    if (p.k_sub == 5 && !p.sub_semi_root && J >= 6 && L[1].nr > RES_NMAX) p.sub5 = IMG_SUB;
    // (b5) ... and k_resident's POLY3 mode (level 1 of at most 2048 rows) keeps level 4 in polynomial form in its
    // workgroups as well when there are six levels or more (ResDesc::p4rows).  Its tail workgroup takes the
    // image rooted at level 4 that the POLY3 mode uses anyway and enters it at level 5 (an image of its own,
    // rooted at level 5, packed levels 5..J a second time: +85 us per hierarchy, more than the cycles gained).
    if (p.sub5 == IMG_NONE && poly3_likely && J >= 6 && L[1].nr <= RES_NMAX &&
        ((p.k_sub == 3 && p.image(IMG_SUB4)) || (p.k_sub == 4 && !p.sub_semi_root)) && L[4].nr <= RES_P4_SEG &&
        L[5].nr <= 64 && !sw.no_res_poly4)
        p.sub5 = p.k_sub == 3 ? IMG_SUB4 : IMG_SUB;
}

// L[1..J]: the levels' shapes
inline LevelPlan plan_levels(const LevelShape* L, int J, const PlanOptions& o, const PlanSwitches& sw) {
    LevelPlanner pl{};
    pl.L = L;
    pl.J = J;
    pl.o = o;
    pl.sw = sw;
    pl.cyc = o.cycle == 'w' || o.cycle == 'v';
    pl.choose_forms();
    LevelPlan p;
    p.J = J;
    p.use_poly = pl.use_poly;
    p.use_lpoly = pl.use_lpoly;
    p.lean_vectors = pl.lean_vectors;
    p.tiny_lo = pl.tiny_lo;
    p.poly.assign((size_t)J + 2, 0);
    p.lpoly.assign((size_t)J + 2, 0);
    p.bpoly.assign((size_t)J + 2, 0);
    p.bdense.assign((size_t)J + 2, 0);
    for (int k = 1; k <= J; ++k) {
        p.poly[(size_t)k] = pl.is_poly(k);
        p.lpoly[(size_t)k] = pl.is_lpoly(k);
        p.bpoly[(size_t)k] = pl.is_bpoly(k);
        p.bdense[(size_t)k] = pl.is_bdense(k);
    }
    pl.plan_solve(p);
    pl.plan_sub(p);
    pl.plan_tails(p);
    return p;
}
