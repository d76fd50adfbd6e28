// Planner of the setup (amg_transfer: ipd_setup.hip, ipd_coarsen.hip, ipd_prolong.hip; csr_spgemm: ipd_sparse.hip):
// from plain sizes, the previous hierarchy's entry counts of the same level and three switches it decides which
// form of mis_set and of the interpolation build a level takes, whether the entry counts of P, P'A and Ac stay on
// the device, how a counted matrix gets its row pointers, and which kernel a product runs on.  The executors walk
// the plan and compare no size against a threshold themselves.  Host-clean, no HIP, no getenv:
// tests/setup_plan_driver.cpp runs it on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "ipd_limits.h"

// IPD_INTERP, IPD_PRODUCT, IPD_NO_MIS_SMALL (ipd_switches.h), read once per amg_transfer / csr_spgemm call
enum InterpSwitch { INTERP_AUTO, INTERP_SINGLE, INTERP_SPLIT, INTERP_BLOCK };
enum ProductSwitch { PRODUCT_AUTO, PRODUCT_ROWS, PRODUCT_TILES };
struct SetupSwitches {
    InterpSwitch interp = INTERP_AUTO;
    ProductSwitch product = PRODUCT_AUTO;
    bool no_mis_small = false;
};
// the values as the environment holds them (nullptr: unset).  Any IPD_INTERP other than split or block is the
// one-kernel form; any IPD_PRODUCT other than rows or tiles leaves the choice to the model.
static inline SetupSwitches setup_switches(const char* interp, const char* product, bool no_mis_small) {
    SetupSwitches sw;
    if (interp) sw.interp = !std::strcmp(interp, "split") ? INTERP_SPLIT : !std::strcmp(interp, "block") ? INTERP_BLOCK : INTERP_SINGLE;
    if (product) sw.product = !std::strcmp(product, "tiles") ? PRODUCT_TILES : !std::strcmp(product, "rows") ? PRODUCT_ROWS : PRODUCT_AUTO;
    sw.no_mis_small = no_mis_small;
    return sw;
}

// ---------------------------------------------------------------------------------------------------------------
// How a counted matrix gets its row pointers and its entry count.  With a lazy count the consumer (a compaction)
// scans the producer's plain counts on its way in (scan_head) while they fit its LDS.  Otherwise producers with
// 256-thread workgroups scan their own counts at the end of the launch (ScanTail) -- the total stays on the device
// (lazy) or the host waits for it -- and one-wave producers are followed by a scan launch, whose total again
// stays on the device or is fetched.
// ---------------------------------------------------------------------------------------------------------------
enum RowCountMode { RC_HEAD, RC_TAIL_LAZY, RC_TAIL_WAIT, RC_SCAN_LAZY, RC_SCAN_TOTAL };
static constexpr const char* ROW_COUNT_NAMES[] = {"HEAD", "TAIL_LAZY", "TAIL_WAIT", "SCAN_LAZY", "SCAN_TOTAL"};
static inline RowCountMode plan_row_count(bool lazy, int nr, bool producer_has_tail) {
    if (lazy && nr <= SCAN_HEAD_MAX) return RC_HEAD;
    if (producer_has_tail) return lazy ? RC_TAIL_LAZY : RC_TAIL_WAIT;
    return lazy ? RC_SCAN_LAZY : RC_SCAN_TOTAL;
}
static inline bool row_count_has_tail(RowCountMode m) { return m == RC_TAIL_LAZY || m == RC_TAIL_WAIT; }

// 256 threads per row (a barrier per step) from WIDE_ROW_MIN entries per row on, one wave below
static inline int row_threads(int nr, long long nnz) { return (nr > 0 && (double)nnz / nr >= WIDE_ROW_MIN) ? 256 : 64; }

// ---------------------------------------------------------------------------------------------------------------
// The ordered product C = X*Y.  Which kernel is expected to finish first (measured on MI355X).  The row kernels
// are a dependent chain per output row, one step per entry of X's row: the one-wave kernel (short rows of Y) takes
// about 0.16 us per entry with the rows of Y prefetched eight deep, the 256-thread kernel 0.35 us + 0.25 us per
// 256 entries of Y's row with a barrier per step; rows are spread over the CUs as LDS allows.  The tile kernel
// walks the padded rows x inner x columns box 16 inner indices at a time -- about 0.9 us per step and wave of
// 256 64-edge tiles, 0.23 us with the 32-edge tiles small products get -- plus 20-40 us for the expansion of
// the operands and the row count.  IPD_PRODUCT=rows|tiles overrides the choice (tests compare the two bit for bit).
// ---------------------------------------------------------------------------------------------------------------
struct ProductShape {   // nnz: an estimate will do under a lazy count (both kernels give the same bits)
    int nr = 0, nc = 0;
    long long nnz = 0;
};
struct ProductPlan {
    bool tiles = false;
    int edge = SPGEMM_TILE;      // tiles: 64, or 32 where few 64-edge tiles would leave most CUs idle
    int threads = 64;            // rows: threads per row
    RowCountMode rows = RC_SCAN_TOTAL;
    size_t bound = 0;            // dense bound nr*nc: sizes C's arrays under a lazy count
    size_t bytes = 0;            // the tile kernel's dense operand and result blocks
    bool modelled = false;       // the choice came from the two model times below
    double xlen = 0.0, ylen = 0.0, t_rows = 0.0, t_tiles = 0.0;   // us
};
static inline size_t plan_round_up(size_t v, size_t q) { return (v + q - 1) / q * q; }
static inline ProductPlan plan_product(const ProductShape& X, const ProductShape& Y, int x_maxrow, ProductSwitch sw,
                                       bool lazy) {
    ProductPlan p;
    const size_t nrp = plan_round_up((size_t)X.nr, SPGEMM_TILE), nkp = plan_round_up((size_t)X.nc, SPGEMM_TILE),
                 ncp = plan_round_up((size_t)Y.nc, SPGEMM_TILE);
    p.bytes = 8 * (nrp * nkp + nkp * ncp + nrp * ncp);
    p.bound = (size_t)X.nr * (size_t)Y.nc;
    p.edge = (nrp / SPGEMM_TILE) * (ncp / SPGEMM_TILE) >= 256 ? SPGEMM_TILE : SPGEMM_TILE / 2;
    p.threads = row_threads(Y.nr, Y.nnz);
    if (X.nr == 0 || X.nc == 0 || Y.nc == 0 || X.nnz == 0 || p.bytes > SPGEMM_TILE_BYTES_MAX)
        p.tiles = false;
    else if (sw != PRODUCT_AUTO)
        p.tiles = sw == PRODUCT_TILES;
    else {
        // (one round of rows: the launch is as slow as its longest row)
        p.modelled = true;
        p.ylen = (double)Y.nnz / Y.nr;
        p.xlen = (X.nr <= 256 * 8) ? std::max((double)X.nnz / X.nr, (double)x_maxrow) : (double)X.nnz / X.nr;
        const bool shortrows = p.ylen < WIDE_ROW_MIN;
        const double lds_rows = std::max(1.0, std::min(shortrows ? 32.0 : 8.0, 160.0 * 1024 / (8.0 * Y.nc + 64)));
        const double row_rounds = std::ceil(X.nr / (256.0 * lds_rows));
        p.t_rows = row_rounds * p.xlen * (shortrows ? 0.16 : 0.35 + 0.25 * std::ceil(p.ylen / 256.0));
        const double tiles = (double)(nrp / SPGEMM_TILE) * (double)(ncp / SPGEMM_TILE);
        const double steps = (double)(nkp / SPGEMM_TILE_K);
        const double t_walk = tiles >= 256.0 ? 20.0 + std::ceil(tiles / 256.0) * steps * 0.9
                                             : std::ceil(4.0 * tiles / 1024.0) * steps * 0.23;
        p.t_tiles = 20.0 + t_walk + (double)p.bytes / 3.0e6;   // (operand block zeroed and written at ~3 TB/s)
        p.tiles = p.t_tiles < p.t_rows;
    }
    p.rows = plan_row_count(lazy, X.nr, p.tiles || p.threads == 256);
    return p;
}
// the model's line of IPD_DEBUG_LEVELS (products the model chose for)
static inline std::string product_plan_line(const ProductShape& X, const ProductShape& Y, const ProductPlan& p) {
    char b[192];
    std::snprintf(b, sizeof(b), "[ipd] product %d x %d x %d: x row %.1f, y row %.1f entries; model rows %.1f us, tiles %.1f us",
                  X.nr, X.nc, Y.nc, p.xlen, p.ylen, p.t_rows, p.t_tiles);
    return b;
}

// ---------------------------------------------------------------------------------------------------------------
// One level's transfer (AMG/transfer.m), in two steps: the number of coarse nodes is known only after the split.
// ---------------------------------------------------------------------------------------------------------------
struct TransferShape {
    int level = 0;            // of A (1-based); the hints are kept for 1 <= level < XFER_HINT_LEVELS
    int N = 0, nnz = 0;       // A
    int bigph = 0, inter = 1;
    long long fnode = 0;      // amg_options
    int hint[4] = {0, 0, 0, 0};   // the last hierarchy's entries of P, P'A, Ac and longest row of P'A on this level (0: none)
};
static inline bool transfer_has_hints(int level) { return level >= 1 && level < XFER_HINT_LEVELS; }
static inline bool transfer_is_bigraph(const TransferShape& s) { return s.level == 1 && s.bigph != 0; }   // transfer.m:19

// Before the split: mis_set as one launch (k_mis_small), by size and switch.  The executor still runs the
// launch-per-step form where no mailbox ticket is granted or the degenerate branch of mis_set.m:30-34 comes up.
static inline bool plan_mis_small(int N, int nnz, const SetupSwitches& sw) {
    return N >= 1 && N <= MIS_SMALL_ROWS && nnz <= MIS_SMALL_NNZ && !sw.no_mis_small;
}

enum InterpForm {
    FORM_BIGRAPH,   // level 1 of a bigraph hierarchy: W = (-Aff)\Afc with Aff diagonal (k_bigph_*)
    FORM_IDEAL,     // inter >= 2: W = -Aff \ Afc by a dense Cholesky (cold path)
    FORM_SPLIT,     // very long rows (filled-in level 2 under dense masks): W2 = X*W1 as a csr_spgemm
    FORM_WAVE,      // one wave per row, pipelined (k_build_W_w)
    FORM_BLOCK      // the barrier-per-neighbour form (k_build_W), kept for the bit-for-bit tests
};
static constexpr const char* INTERP_FORM_NAMES[] = {"BIGRAPH", "IDEAL", "SPLIT", "WAVE", "BLOCK"};
struct TransferPlan {
    InterpForm form = FORM_WAVE;
    int block_threads = 64;   // FORM_BLOCK: threads per row
    // Lazy counts: where the dense bounds are small the entry counts of P (lazy) and of P'A and Ac (lazy_prod)
    // stay on the device until all are fetched in ONE round trip at the end of the level.  The products' kernel
    // choice meanwhile runs on the previous hierarchy's counts of the same level (both kernels give the same bits).
    bool lazy = false, lazy_prod = false;
    RowCountMode p_rows = RC_SCAN_TOTAL;
    size_t p_bound = 0, pta_bound = 0, ac_bound = 0;   // dense bounds that size P, P'A and Ac under lazy counts
};
static inline TransferPlan plan_transfer(const TransferShape& s, int Nc, const SetupSwitches& sw) {
    TransferPlan p;
    const bool bigraph = transfer_is_bigraph(s);
    const size_t N = (size_t)s.N, nc = (size_t)Nc;
    p.pta_bound = nc * N;
    p.ac_bound = nc * nc;
    // (level 1 of a bigraph: P holds a sub-pattern of A's F rows and one entry per C row)
    p.p_bound = bigraph ? std::min((size_t)s.nnz + N, N * nc) : N * nc;
    // the lazy gate: bounds within SPGEMM_LAZY_MAX, and estimates for every product whose count is not waited for
    // (P'A and Ac: hint[1], hint[2]; P as well: hint[0]).  The bigraph level's fill is its own consumer and has
    // the head scan only.
    const bool bounds_ok = N * nc <= SPGEMM_LAZY_MAX && p.ac_bound <= SPGEMM_LAZY_MAX;
    p.lazy_prod = transfer_has_hints(s.level) && s.hint[1] > 0 && s.hint[2] > 0 && bounds_ok;
    p.lazy = p.lazy_prod && s.hint[0] > 0 && (!bigraph || s.N <= SCAN_HEAD_MAX);
    const double row = (double)s.nnz / std::max(s.N, 1);
    if (bigraph)
        p.form = FORM_BIGRAPH;
    else if (s.inter >= 2)
        p.form = FORM_IDEAL;
    else if (sw.interp == INTERP_AUTO ? row >= SPLIT_ROW_MIN : sw.interp == INTERP_SPLIT)
        p.form = FORM_SPLIT;
    else
        p.form = sw.interp == INTERP_BLOCK ? FORM_BLOCK : FORM_WAVE;
    p.block_threads = row >= WIDE_ROW_MIN ? 256 : 64;
    // the counting launches of the bigraph, ideal and product forms have 256-thread workgroups; k_build_W(_w)'s
    // workgroups cannot scan
    p.p_rows = plan_row_count(p.lazy, s.N, p.form == FORM_BIGRAPH || p.form == FORM_IDEAL || p.form == FORM_SPLIT);
    return p;
}
static inline std::string transfer_plan_line(const TransferShape& s, int Nc, const TransferPlan& p) {
    char b[256];
    std::snprintf(b, sizeof(b), "transfer level %d N=%d nnz=%d Nc=%d form=%s threads=%d lazy=%d lazy_prod=%d rows=%s "
                  "p_bound=%zu pta_bound=%zu ac_bound=%zu", s.level, s.N, s.nnz, Nc, INTERP_FORM_NAMES[p.form],
                  p.block_threads, (int)p.lazy, (int)p.lazy_prod, ROW_COUNT_NAMES[p.p_rows], p.p_bound, p.pta_bound,
                  p.ac_bound);
    return b;
}
