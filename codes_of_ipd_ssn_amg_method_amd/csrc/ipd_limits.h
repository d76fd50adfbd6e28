// Sizes and limits shared by the device code and the level planner (ipd_level_plan.h).  Host-clean:
// the planner's CPU test compiles it with a plain C++ compiler.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define IPD_HD_INLINE __host__ __device__ __forceinline__
#else
#define IPD_HD_INLINE inline
#endif

// threads per block of every phase kernel and of the single-workgroup kernels (their helpers
// share the block reductions, so it is one constant).  Measured, 1024 -> 512: regime-D V cycle
// 0.194 -> 0.190 ms, tree-mask W cycle 0.503 -> 0.431 ms, m=n=1024 Class 1 / Class 2 driver runs
// 1.53 / 0.74 -> 1.47 / 0.70 s, m=n=4096 Class 1 5.33 -> 4.97 s (only the bandwidth-bound
// m=n=2048 regime-D cycle loses: 0.328 -> 0.342 ms); 256: 0.234 ms and the sub-cycle kernel no
// longer takes 300-1000-row roots (Class 1 run 20 s).
static constexpr int BT = 512;

static constexpr int STAGE_MAX = 7680;   // vector entries staged in LDS (60 KiB)

// matrix entries in flight per lane and batch (one 4-entry vector of the padded format).
// 8 was slower on every workload (m=n=1024 Class 1 run 1.58 -> 1.55 s, tree-mask W cycle
// 0.532 -> 0.503 ms): short rows fill 3-6 of the slots and the rest are clamped dummy loads.
static constexpr int ROW_U = 4;

// Thresholds of the launch path's rules (ipd_launch_plan.h, where the measurements behind them are recorded)
static constexpr double QUEUED_NNZ_MAX = 6000.0;   // matrix entries of a phase queued into the fused program
static constexpr int RRC_T1_NNZ_MAX = 1 << 18;     // entries of T1 = P'A up to which residual + restriction run fused
static constexpr int PAD_ROWS_MAX = 65535;         // rows of a padded copy (16-bit columns)
static constexpr double PAD_AVG_MIN = 0.5;         // mean off-diagonal row length from which a level is padded
static constexpr double PAD_SLACK_FACTOR = 1.3, PAD_SLACK = 16.0;   // pad width S <= 1.3 * mean + 16
static constexpr int PAD_BATCHES = 8;              // ROW_U batches per lane of a padded row before the chip-filling rule
static constexpr int PCG_LANES_MAX = 64;           // lanes per row of the coarsest level's PCG

// Thresholds of the setup's rules (ipd_setup_plan.h; the measurements behind them are recorded there and where
// the kernels they choose between are defined)
static constexpr size_t SPGEMM_LAZY_MAX = size_t(1) << 21;   // dense bound nr*nc up to which a product's arrays are sized by it
static constexpr int SCAN_HEAD_MAX = 4096;                   // rows a consumer scans itself (scan_head: ScanHeadLds::rp)
static constexpr int MIS_SMALL_ROWS = 1024;                  // rows / entries of a level up to which mis_set is one launch
static constexpr int MIS_SMALL_NNZ = 40000;                  // (k_mis_small: a thread per node, the strong lists in LDS)
static constexpr double SPLIT_ROW_MIN = 256.0;               // mean row length from which the interpolation is built as a product
static constexpr double WIDE_ROW_MIN = 96.0;                 // mean row length from which a row gets 256 threads, not one wave
static constexpr int SPGEMM_TILE = 64, SPGEMM_TILE_K = 16;   // the tile product's output tile edge and inner-index tile
static constexpr size_t SPGEMM_TILE_BYTES_MAX = size_t(12) << 30;     // dense operand blocks of the tile product
static constexpr size_t DENSE_SCRATCH_BYTES_MAX = size_t(2) << 30;    // dense rows of a row product / an interpolation build
static constexpr int SPGEMM_COLS_MAX = 16384;                // columns of a row product (one LDS accumulator row)
static constexpr int XFER_COARSE_MAX = 8192;                 // coarse nodes of a non-bigraph level (two LDS rows in k_build_W*)
static constexpr int XFER_HINT_LEVELS = 40;                  // levels ipd_ctx::xfer_hint keeps the last hierarchy's counts of

// the drivers (ipd_apd_create): rows and columns of the transport problem; the cost out of point clouds
// (ipd_cost_plan.h): coordinates per point
static constexpr int IPD_APD_SIDE_MAX = 16384;
static constexpr int IPD_COST_DIM_MAX = 16;

// the KKT operators (ipd_kkt.hip, ipd_asat.hip; their host rules: ipd_kkt_plan.h)
static constexpr int AX_TR = 256;         // Ax: tile rows
static constexpr int AX_TC = 16;          // Ax: tile columns
static constexpr int AX_LD = AX_TR + 16;  // Ax: padded column stride of the LDS tile (bank spread)
static constexpr int ATY_TC = 16;         // Aty: columns per workgroup
static constexpr int ASAT_TILE = 64;      // ASAt: edge of a mask tile (one 64-bit word per row or column of it)
static constexpr int PHI_PARTS_MAX = 1024;   // invHHt: most partial sums of |phi|^2 (k_inv_hht_combine's one workgroup adds them)
// ASAt's one-launch route (k_asat_small): mask words a thread holds for its row, workgroups the chained scan
// can look back over (one lane per predecessor), the largest entry count of the previous call that takes it,
// and the count it posts when a spin gave up
static constexpr int ASAT_SMALL_WORDS = 16;
static constexpr int ASAT_SMALL_WGS = 64;
static constexpr int ASAT_SMALL_HINT_MAX = 65536;
static constexpr int ASAT_GAVE_UP = 2147483647;

// levels a single-workgroup image (SolveDesc) holds
static constexpr int SOLVE_ML = 24;
// An LDS image (ipd_level_plan.h): the planner admits levels while the predicted dynamic LDS stays within the
// budget; the kernels that run out of an image opt in to a little more (an image's operator copy, SolveDesc::bm_src,
// goes behind it).  The head of an image is the descriptor and its relocation table of RELOC_MAX words:
// SOL_HEAD == sol_r16(sizeof(SolveDesc)) + sol_r16(4 * RELOC_MAX), asserted where SolveDesc is defined.
static constexpr size_t IMAGE_LDS_BUDGET = (size_t)150 * 1024;
static constexpr size_t IMAGE_LDS_OPTIN = (size_t)156 * 1024;
static constexpr int RELOC_MAX = 640;
static constexpr size_t SOL_HEAD = 12592;

// most iterations the one-launch AMG-PCG (k_pcg_small) is asked for: at ~0.3 ms per iteration a launch
// then cannot outlast ~0.3 s; a call with a larger maxit runs as launches
static constexpr int PCG_SMALL_MAXIT = 1000;

// widest block of right-hand sides (ipd_block.hip, ipd_block_krylov.hip; chunking: ipd_krylov_plan.h).
// W = 16 was dropped: its smoother and loop-top instantiations spill (VGPRs and SGPRs past the 256 / 106
// a 512-thread workgroup gets; -Rpass-analysis=kernel-resource-usage), W <= 8 do not
static constexpr int BLK_WMAX = 8;

// dense thread-per-row levels (SolveLevel::blk_dense, ipd_cycle.hip): 24 values per lane: the register
// budget of the tail (the resident kernels' worker paths set the kernels' allocation; the tail must stay
// below it) -- the same storage serves the lane-map entries.
static constexpr int BDENSE_Q = 24;
IPD_HD_INLINE int bdense_lanes(int N) { return N > 64 ? 4 : 8; }   // == lanes_per_row(N), 33..96 rows
IPD_HD_INLINE int bdense_pad(int N) {
    const int g = 4 * bdense_lanes(N);
    return (N + g - 1) / g * g;
}
IPD_HD_INLINE int bdense_ld(int N) {
    const int Lr = bdense_lanes(N), p = bdense_pad(N);
    return p % (2 * Lr) == Lr ? p : p + Lr;   // p is a multiple of 4 Lr
}

// level-resident kernel (ipd_resident.h)
static constexpr int RES_WAVES = BT / 64;     // row slots per block and workgroup (one wave per row)
static constexpr int RES_NMAX = 4 * BT;        // rows per level (fixed LDS slots)
static constexpr int RES_P4_SEG = 128;         // ... of ResDesc::p4rows: 128 + 128 + 64
static constexpr int RES_TAIL_MAX = 64;        // rows of the redundantly solved tail level
static constexpr size_t RES_LDS_BYTES = sizeof(double) * ((size_t)9 * RES_NMAX + RES_NMAX / 2 + 3 * RES_TAIL_MAX + 14 * RES_WAVES + 12 + 6 * RES_WAVES + 8 + RES_WAVES * RES_WAVES);   // (... sums, publish slots, own scalars; fail word and stamps; rowp: 12 ints per wave; stamps by class; the full shape's third buffer of row totals)
static constexpr size_t RES_LDS_MAX = IMAGE_LDS_OPTIN;   // dynamic LDS a resident launch may ask for (its own or its tail image's)

// mask-form resident kernel (ipd_resident_big.h)
static constexpr int RB_NMAX = 8 * BT;                 // rows of level 1
static constexpr int RB_HALF = 4 * BT;                 // rows of a block of level 1 / of level 2
static constexpr int RB_N3MAX = 2 * BT;                // rows of the polynomial level 3 (DEEP)
static constexpr int RB_N4MAX = BT / 2;                // rows of the remote tail's root level (DEEP)
static constexpr int RB_N5MAX = BT / 4;                // rows of the tail's root level when level 4 is resident too (POLY4)
static constexpr int RB_RPW_MAX = 2;                   // rows of a block per wave
// LDS (doubles): E2, TU, P3C / RR2, E1S, XS, reductions, publish slots, own-row constants, fail word;
// DEEP: R3, E3 (RB_N3MAX each), E4, R4 (RB_N4MAX each), E5 (RB_N5MAX), 128 partial sums of the polynomial passes
static constexpr size_t RB_LDS_DOUBLES = (size_t)2 * RB_NMAX + 3 * RB_HALF + 2 * RES_WAVES +
                                         2 * 8 * RB_RPW_MAX + 20 * 8 * RB_RPW_MAX + 8 +
                                         2 * RB_N3MAX + 2 * RB_N4MAX + RB_N5MAX + 128;
static constexpr size_t RB_LDS_BYTES = sizeof(double) * RB_LDS_DOUBLES;

// Hybrid_AMG's routing (ipd_hybrid_plan.h): a component of more than HYBRID_N0 nodes gets its own AMG solve, the
// others are solved together, one workgroup per block with the block's dense copy in LDS (Hybrid_AMG.m:51-53, :85)
static constexpr int HYBRID_N0 = 100;
// a component's mask form is only of use beyond k_resident's 2048 rows (the mask-form kernel's deep mode)
static constexpr int RES_MASK_MIN_ROWS = 2048;
static constexpr size_t HYBRID_SMALL_LDS_OPTIN = (size_t)96 * 1024;   // dynamic LDS k_small_blocks opts in to
// k_small_blocks' dynamic LDS for blocks of up to nb rows: the nb x (nb + 1) matrix and the right-hand side
static constexpr size_t hybrid_small_lds(int nb) { return sizeof(double) * ((size_t)nb * (nb + 1) + nb); }
static_assert(hybrid_small_lds(HYBRID_N0) <= HYBRID_SMALL_LDS_OPTIN, "a small block of HYBRID_N0 rows must fit the LDS opted in to");
