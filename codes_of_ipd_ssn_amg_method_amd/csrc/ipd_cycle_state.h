// Host side of the cycle, shared by its units: the per-level run state, CycleState, and the host functions that
// cross from one unit to another.  A kernel is launched only by the unit that defines it, so another unit goes
// through one of these functions.
//   ipd_cycle.hip           the launch path: its kernels, amg_prepare_levels, amg_cycle, the Class_AMG loop
//   ipd_image.hip           the LDS images and the polynomial operators: the pack kernels and pack_image
//   ipd_small.hip           the single-workgroup kernels and their launches
//   ipd_resident_host.hip   the resident kernels' table, plans, launch and attach functions
//   ipd_resident_k*.hip     the resident kernels' instantiations
//   ipd_cycle_bench.hip     the measurement hooks
#pragma once

#include <cstdlib>

#include "ipd_amg_internal.h"
#include "ipd_cycle_args.h"
#include "ipd_resident_plan.h"

struct LevelRun {  // per-level run state kept next to Level
    LevelDev dev;
    bool e_zero = true;      // the iterate is identically zero and is not materialised
    LaunchLevel plan;        // how the level's phases run on the multi-launch path (ipd_launch_plan.h)
    int maxoff = 0;          // longest off-diagonal row (k_levels_prepare)
    XferArgs restrict_args;  // r_{k+1} = P' rr_k   (stored on level k)
    XferArgs prolong_args;   // e_k += P e_{k+1}
    PcgArgs pcg;             // coarsest only
};

// The resident solve kernels' plan and run state: ipd_resident_host.hip defines it and is the only code that looks
// inside -- the rest of the host asks whether a plan is active (resident_active).
struct ResidentState;

struct CycleState {
    std::vector<LevelRun> run;  // 1-based
    double* hist = nullptr;
    // row-block sharding: `shard_ranks` owners per row range.  In emulate mode
    // one process plays all owners back to back on the shared vectors (the all-gather is
    // then implicit) -- used by the single-GPU test of the slicing logic.
    int shard_ranks = 1;
    int shard_rank = 0;
    bool shard_emulate = false;
    int shard_min_rows = 256;
    int num_cu = 256;
    // fused single-workgroup program under construction (flushed before any big launch)
    FusedProg pending;
    size_t pending_lds = 0;
    CycleState() { pending.n = 0; }
    // The LDS images of the single-workgroup kernels (ipd_level_plan.h) by role: the whole solve (k_solve_small,
    // k_pcg_small), the sub-cycle rooted at level k_sub (k_subcycle), and the images rooted at level 3 (no sub-cycle:
    // k_sub == 0) and at level 4 (beside a sub-cycle rooted at level 3: `three` mode) that the resident kernels' tail
    // workgroup takes alone
    struct Image {
        SolveDesc* desc = nullptr;
        size_t lds = 0;   // dynamic LDS of a launch
        size_t bm = 0;    // ... and what the image's operator copy needs on top of it (SolveDesc::bm_src; 0: none)
    };
    Image img[IMG_NONE];
    double* solve_out = nullptr;   // the whole-solve kernel's outputs
    bool small_ok = false;
    bool solve_cached = false;
    // matrix-free level-1 operator (bit mask + scale vectors), see k_smooth_mask
    bool mask_ok = false;
    MaskOp maskop{};
    int k_sub = 0;                 // root of the IMG_SUB image (0 = none)
    bool sub_semi_root = false;    // ... which is semi-cached (rows from L2)
    std::vector<int> level_forms;  // per level, over all images packed: see ipd_amg_level_forms
    struct PolyOp {                // block-wide polynomial operators packed for the images (ipd_amg_poly_operator)
        const double* M = nullptr;
        const double* W = nullptr;
        int LD = 0, N = 0, Nc = 0;
    };
    std::vector<PolyOp> poly_ops;
    struct RowsOp {                // row-layout polynomial operators of the resident kernels (ipd_amg_packed_operator)
        const double* M = nullptr; // [N + Nc][ld], W (N + Nc entries) right behind
        int ld = 0, seg = 0, N = 0, Nc = 0;
    };
    std::vector<RowsOp> rows_ops;  // per level: form 64 (level 3 / 4 of k_resident's `three` mode or of DEEP mode)
    RowsOp poly2_op;               // form 128: level 2 composed over a visit
    ImageRole sub5 = IMG_NONE;     // the image whose levels 5..J serve a resident kernel's tail rooted at level 5 (POLY4)
    double* x2 = nullptr;
    // The resident solve kernels' plan and run state.  Never null in a state that a hierarchy holds: amg_prepare_levels,
    // the one creator of a CycleState, calls prepare_resident (which makes it) before it publishes the state in
    // ipd_amg::cyc.  (Uniquely owned; a shared_ptr because it deletes an incomplete type with the deleter it was made
    // with, as ipd_amg::cyc does for CycleState itself.)
    std::shared_ptr<ResidentState> res;
    hipGraphExec_t gexec[2] = {nullptr, nullptr};  // captured Class_AMG loop bodies (x->x2, x2->x)
    const double* gb = nullptr;                    // right-hand side the graphs were captured for
    ~CycleState() {
        for (auto& g : gexec)
            if (g) (void)hipGraphExecDestroy(g);
    }
};

inline CycleState* state_of(ipd_amg* h) { return h->cyc.get(); }

// ---- ipd_cycle.hip --------------------------------------------------------------------------
// the planners' switches, read at the call in which they take effect; the levels as the planners look at them
PlanSwitches read_plan_switches();
std::vector<LevelShape> level_shapes(const ipd_amg* h, const CycleState* st);
void flush_fused(ipd_ctx* ctx, CycleState* st);
// one smoother sweep on level k: Jacobi = one launch, bigraph GS = two half launches
void launch_sweep(ipd_amg* h, CycleState* st, int k, int isnsp, bool post);
void launch_top(ipd_amg* h, CycleState* st, const double* b, const double* x, const double* e, double* xnew, bool first);
// one Class_AMG loop body (Class_AMG.m:96-105): x_out = x_in + cycle(b - A x_in)
void enqueue_loop_body(ipd_amg* h, CycleState* st, const double* b, const double* xin, double* xout);
// dev->pci, pva, diag: a padded off-diagonal copy of A with stride S, the caller's own, out of the hierarchy's arena
void build_padded_private(ipd_amg* h, const Csr& A, int S, LevelDev* dev);
// The bit-mask form of level 1 (n F rows, m C rows) out of the hierarchy's arena: the scales alpha = q^2 / tk and
// beta = p^2, the rows' bit masks, the diagonal.  False (and *mo untouched) unless every entry of A_1 has the
// rank-one form.  `bad`: one int of scratch.
bool build_maskop(ipd_amg* h, const double* p_dev, const double* q_dev, int m, int n, double tk, int* bad, MaskOp* mo);

// ---- ipd_image.hip -------------------------------------------------------------------------
// packs image `spec` as image_layout lays it out and stores it in st by its role
void pack_image(ipd_ctx* ctx, ipd_amg* h, CycleState* st, const std::vector<LevelShape>& shapes, const LevelPlan& plan, const ImageSpec& spec);
// The polynomial form of level k packed into the hierarchy's arena: LD-row column-major [Mr | Me | Mc] for the
// single-workgroup images, or (rows) row-major [N + Nc][rows_ld] with Mr, Me, Mc at columns 0, rows_seg and
// 2 rows_seg, as the resident kernels take it.  W lies right behind M.
struct BPolyEntry;   // the pack kernels' argument record
struct BPolyPack {
    double* M = nullptr;
    double* W = nullptr;
    std::shared_ptr<const BPolyEntry> ops;   // the pack's operands (scratch: valid until the call scope ends)
};
BPolyPack pack_bpoly(ipd_ctx* ctx, ipd_amg* h, CycleState* st, int k, int isnsp, int LD, bool rows, int rows_seg, int rows_ld);
// level 2 composed over a whole visit, into the Me segment and W of a row-layout pack of that level
void bpoly_compose(ipd_ctx* ctx, const BPolyPack& b);
// what a row-layout pack holds, for ipd_amg_packed_operator; record_rows_op: as level k of st->rows_ops
CycleState::RowsOp rows_op(const BPolyPack& b);
void record_rows_op(CycleState* st, const ipd_amg* h, int k, const BPolyPack& b);

// ---- ipd_small.hip -------------------------------------------------------------------------
void optin_small_kernels(ipd_ctx* ctx);   // the single-workgroup kernels may ask for IMAGE_LDS_OPTIN of dynamic LDS
// the whole solve phase (cycles == 0) or `cycles` cycles without stopping rules as one single-workgroup launch
void launch_solve_small(ipd_ctx* ctx, CycleState* st, const double* b_dev, double* x, int cycles);
// everything from level st->k_sub down as one workgroup on the IMG_SUB image
void launch_subcycle(ipd_ctx* ctx, CycleState* st, bool keep_e);

// ---- ipd_resident_host.hip -----------------------------------------------------------------
// Plans k_resident for the hierarchy, does the device work the plan calls for and makes st->res (amg_prepare_levels)
void prepare_resident(ipd_amg* h, CycleState* st, const std::vector<LevelShape>& shapes, const PlanSwitches& sw);
void print_resident_summary(std::FILE* f, const CycleState* st);   // the "resident=..." field of the debug line
bool resident_active(const CycleState* st);   // a plan is active: the solve phase is one launch of co-resident workgroups
// Runs the whole solve (fixed_cycles == 0) or exactly fixed_cycles loop bodies on the iterate in x (in: guess,
// out: result).  Returns false when the kernel could not be used (another resident kernel is running, or a spin
// gave up): x is then unspecified and the caller takes the multi-launch path.  `ms`: device time of the launch
// (HIP events), optional.
bool run_resident(ipd_amg* h, CycleState* st, const double* b_dev, double* x, int fixed_cycles,
                  std::vector<double>* out_host, float* ms, long long* dbg_dev = nullptr);
