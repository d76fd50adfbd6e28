// Host side of the drivers, shared by their units: the handle, the records the passes hand back, and the host
// functions that cross from one unit to another.  A kernel is launched only by the unit that defines it, so
// another unit goes through one of these functions.
//   ipd_driver.hip       workspace creation, apd_iterate, the step-reuse test, the ABI
//   ipd_apd_passes.hip   the four pass families of an iteration (begin, eval, merit, end) and their epilogues
//   ipd_apd_warm.hip     the A-ADMM warm start
//   ipd_plan.hip         the transport plan as a sparse matrix, out of and into the workspace
//   ipd_plan_apply.hip   the plan applied to a thin dense matrix
//   ipd_cost.hip         the cost matrix from point clouds
//   ipd_point_grad.hip   the gradient of the transport cost in the point positions
//   ipd_dual.hip         the c-transform of the multiplier, the dual value and the duality gap
//   ipd_round.hip        the iterate rounded to a feasible plan, its exact cost
//   ipd_round_nw.hip     the rounding's sparse correction: north-west corner along a given order
//   ipd_bracket.hip      both certificates of a state in one call; the drivers' probe of the certified gap
#pragma once

#include <functional>
#include <limits>

#include "ipd_amg_internal.h"
#include "ipd_hybrid_state.h"
#include "ipd_apd_script.h"
#include "ipd_apd_tiles.h"
#include "ipd_dual_geo.h"

// device-side scalar results (read back through pinned memory)
struct ApdScal {
    double normF2, lam2, wlk_lam, prox2, z2, zmp2, count, fold_zeta;  // eval
    double kx2, ky2, kz2, kl2, fx;                                     // end
};

struct EvalRes {
    double normF = 0, lam2 = 0, wlk_lam = 0, prox2 = 0, z2 = 0, zmp2 = 0, fold_zeta = 0;
    long long E = 0;
};

struct ipd_apd {
    ipd_ctx* ctx = nullptr;
    std::unique_ptr<Arena> arena;
    int cls = 1, m = 0, n = 0, M = 0, L = 0;
    size_t mn = 0, U = 0;
    Prob P{};
    Geo geo{};
    double mu = 0.0;
    // problem data
    double *c = nullptr, *gama = nullptr, *phi = nullptr, *p = nullptr, *q = nullptr, *b = nullptr;
    // workspace; the x block is the first mn entries of u and v (class 2: of uk = [xk;yk;zk])
    double *u = nullptr, *u2 = nullptr, *v = nullptr, *w = nullptr;
    double *lam = nullptr, *lam_a = nullptr, *lam_b = nullptr, *wlk = nullptr;
    double *F_a = nullptr, *F_b = nullptr, *zeta = nullptr, *negF = nullptr, *tmask = nullptr;
    uint8_t* s = nullptr;
    double *lpart = nullptr, *rpart = nullptr, *spart = nullptr;
    ApdScal* dscal = nullptr;
    double* fpart = nullptr;
    int* counter = nullptr;
    double* merit = nullptr;
    bool merit3 = false;   // of the last ipd_apd_run -- class 1, prob 3: the merit needs |zk|^2 and |zk - prox(zk)|^2 (:186)
    double *phi_l = nullptr, *phi_part = nullptr;  // Ax(phi), partial sums of |phi|^2
    int phi_npart = 0;
    ipd_cost_stats cost_stats{};   // min, max, sum of c: from the build out of points, or on demand (ipd_apd_get_cost)
    bool have_cost_stats = false;  // (c never changes after the create)
    // matrix-free (ipd_apd_create_points_free): c stays nullptr, the coordinates live in the
    // arena and cost_src describes them to the passes that read c(i,j).  A stored workspace made from points
    // (ipd_apd_create_points) fills cost_src too, cost_free false: ipd_point_grad.hip differentiates in them
    bool cost_free = false;
    CostSrc cost_src{};
    int cost_dim = 0, cost_metric = 0, cost_scale = 0;   // of the specification; 0 for a workspace from a host c
    // ipd_apd_dual: what the one check of a c-transform's divider found, [0] q (side 0), [1] p (side 1):
    // 0 not looked at yet, 1 every entry positive and finite, -1 refused
    int8_t dual_divider[2] = {0, 0};
    // script variables
    int k = 0;
    double bk = 1.0;
    double ak = 0, bk1 = 0, tk = 0;  // of the iteration opened by begin()
    bool have_kkt = false;
    double kkt0[4] = {0, 0, 0, 0};   // KKT_xk(1), KKT_lk(1), KKT_yk(1), KKT_zk(1)
    double kkt[4] = {0, 0, 0, 0};
    double fval = 0.0;
    bool converged = false;
    std::vector<double> h_fx, h_kx, h_kl, h_ky, h_kz, h_ssn;
    std::vector<ipd_ssn_rec> recs;
    long long sum_amg = 0, total_amg = 0, fail_amg = 0, max_amg = 0;
    int restarts = 0;
    // row f3: hierarchies of the previous Newton step and what its system was built from
    StepDonors step;
    bool krylov = false;   // ipd_apd_set_krylov: inner_solver 4 runs AMG-PCG behind Hybrid_AMG / AMG4POT
    bool step_reuse = true, have_prev = false;
    double prev_bk1 = 0.0, prev_tk = 0.0;
    size_t s_words = 0;
    unsigned long long *s_prev = nullptr, *t_prev = nullptr;
    int* step_changed = nullptr;
    // the stopping rule on the certified gap (ipd_apd_set_gap_rule): the rule, whether a probe stopped the loop, the
    // best lower bound of the probes so far with the multiplier that attains it (L entries of the arena, made by the
    // first set) and one record per probe
    bool gap_on = false, gap_stopped = false, gap_have_lam = false;
    ipd_gap_rule gap_rule{};
    double gap_best = -std::numeric_limits<double>::infinity();
    double* gap_lam = nullptr;
    std::vector<ipd_gap_rec> gap_recs;
    // the rounding's correction (ipd_apd_set_correction): the mode, the two orders on the device
    // (m and n entries of the arena, made by the first set that gives one; identity while corr_has_* is false), a
    // list of m + n entries per side (made by the first set of a mode other than 0) and what the last rounding or
    // bracket call used -- corr_last_side says whose list that is
    int corr_mode = 0;
    bool corr_has_row = false, corr_has_col = false;
    int32_t *corr_row = nullptr, *corr_col = nullptr;
    int32_t *nw_i[2] = {nullptr, nullptr}, *nw_j[2] = {nullptr, nullptr};
    double* nw_g[2] = {nullptr, nullptr};
    ipd_correction_info corr_last{};
    int corr_last_side = 0;
    int nblk() const { return (int)apd_nblk(geo); }
};

inline Parts parts_of(const ipd_apd* h) {
    Parts pt;
    pt.g = h->geo;
    pt.lpart = h->lpart;
    pt.rpart = h->rpart;
    pt.spart = h->spart;
    pt.nblk = h->nblk();
    return pt;
}

inline void copy_dev(ipd_apd* h, double* dst, const double* src, size_t n) {
    IPD_HIP(hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToDevice, h->ctx->stream));
}

namespace {   // as k_tiles: the calling unit's own instantiation

template <class Op>
void launch_tiles(ipd_apd* h, const Op& op) {
    const Geo& g = h->geo;
    hipLaunchKernelGGL(k_tiles<Op>, dim3(g.nib, g.njg), dim3(256), 0, h->ctx->stream, op, g,
                       h->lpart, h->rpart, h->spart);
    IPD_KERNEL_CHECK();
}

// f(cs) with the cost source of the workspace, CostStored{} or CostFree<D>{...}: every host function that launches
// an op reading c picks the op's instantiation through this
template <class F>
void with_cost_source(const ipd_apd* h, F&& f) {
    if (!h->cost_free) return f(CostStored{});
    switch (h->cost_src.dim) {
        case 1: return f(CostFree<1>{h->cost_src});
        case 2: return f(CostFree<2>{h->cost_src});
        case 3: return f(CostFree<3>{h->cost_src});
        default: throw IpdError(IPD_E_LIMIT, COST_FREE_TEXT[COST_FREE_DIM]);
    }
}
static_assert(COST_FREE_DIM_MAX == 3, "with_cost_source instantiates D = 1, 2, 3");

}  // namespace

// ---- ipd_driver.hip ------------------------------------------------------------------------
// Fills the device arrays of a workspace under construction: c (mn), phi_ones (mn, to be set to ones; nullptr
// when the workspace has no phi or the caller gave one), *st the statistics of c.  A throw abandons the create.
using ApdCostFill = std::function<void(double* c_dev, double* phi_ones_dev, ipd_cost_stats* st)>;
// The one body of ipd_apd_create and ipd_apd_create_points.  Allocates and uploads everything but c: fill == nullptr
// uploads d->c (and needs d->phi for class 2), otherwise fill makes c (and the phi the caller left out).
// Matrix-free, the third way: nothing mn-sized is allocated for c.  Called last with the workspace under
// construction; it puts the coordinates into h->arena and sets h->cost_free, cost_src and cost_stats (and fills
// phi_ones_dev as ApdCostFill does).
using ApdCostFree = std::function<void(ipd_apd* h, double* phi_ones_dev)>;
void apd_create_common(ipd_ctx* ctx, const ipd_apd_data* d, const ApdCostFill* fill, ipd_apd** out,
                       const ApdCostFree* free_fill = nullptr);
// the script variables after a new state went in: what ipd_apd_set_state does besides the uploads
// (k, the KKT reference, the records and the AMG counters start over; bk, lk, histories stay)
void apd_restart_script(ipd_apd* h);

// ---- ipd_apd_passes.hip --------------------------------------------------------------------
size_t apd_fpart_len(int L);   // doubles of ipd_apd::fpart, the evaluation epilogue's per-workgroup partials
// wk, wlk of iteration k; sets h->ak, bk1, tk                    Class1 :113-126, Class2 :110-120
void apd_begin(ipd_apd* h, int k);
// one pass at lam_base (+ step*zeta): F -> F_out, multiplier -> lam_out, mask -> h->s.  merit3: the pass also
// sums |zk|^2 and |zk - prox(zk)|^2 (class 1)
EvalRes apd_eval(ipd_apd* h, bool merit3, const double* lam_base, const double* zeta, double step, double* lam_out,
                 double* F_out, const double* F_old);
// merit cFk at lam_base + step[k]*zeta for MK steps (class 1 prob < 3 and class 2)
void apd_merit(ipd_apd* h, const double* lam_base, const double* zeta, const double step[MK], double merit[MK]);
// uk1/vk1 (from_w) and the KKT residuals of the iterate at multiplier `lam`
void apd_end(ipd_apd* h, bool from_w, const double* src_u, const double* lam, double out_kkt[4], double* fx);
// device time of `reps` evaluation passes at h->lam, without their epilogue
float apd_bench_eval(ipd_apd* h, bool merit3, int reps);

// ---- ipd_apd_warm.hip ----------------------------------------------------------------------
// A-ADMM warm start                       warmup_class1.m:22-96 / warmup_class2.m:19-100
void apd_warmup(ipd_apd* h, double res, long long maxit);

// ---- ipd_cost.hip --------------------------------------------------------------------------
// the largest entry of the unscaled cost of device coordinates (scale = 1 divides by it); IPD_E_ARG when it is 0 or not
// finite.  The caller holds a CallScope; the stream has been waited for afterwards.
double apd_cost_largest(ipd_ctx* ctx, int metric, int dim, int m, int n, const double* xs_dev, const double* ys_dev);

// ---- ipd_dual.hip --------------------------------------------------------------------------
// (the certificate itself is reached through the C ABI, ipd_apd_dual and ipd_apd_dual_dev: it reads the workspace
// through the handle above, remembers its divider check in ipd_apd::dual_divider and keeps every temporary in the
// context's scratch arena.  ipd_bracket.hip walks c itself and has these launch what ipd_dual.hip defines.)
constexpr int APD_STATS_DOUBLES = 16;   // doubles a device copy of ipd_dual_stats or ipd_round_stats takes
bool apd_dual_cap_on(const ipd_apd* h);                // class 1 with finite gama
void apd_dual_check_divider(ipd_apd* h, int side);     // IPD_E_ARG unless q (side 0) resp. p (side 1) is > 0 and finite
// k_du_fin: the partials (pv, pi) of a transform of `side` and the held entries of lam_dev -> lam_out_dev (L), arg_dev
// (du_out_rows entries or nullptr)
void apd_dual_finish(ipd_apd* h, int side, const double* pv, const int* pi, const double* lam_dev, double* lam_out_dev,
                     int32_t* arg_dev);
// k_du_eval: one evaluation of lam_eval into walk_blocks partials
void apd_dual_eval(ipd_apd* h, const double* lam_eval, int primal, DuEvalPart* part);
// k_du_last: an evaluation's partials -> *out_dev (device, APD_STATS_DOUBLES doubles)
void apd_dual_last(ipd_apd* h, const DuEvalPart* part, const double* lam_eval, int primal, ipd_dual_stats* out_dev);

// ---- ipd_round.hip -------------------------------------------------------------------------
// (ipd_apd_round and ipd_apd_round_dev run the four stages below for one side, ipd_bracket.hip runs pass A once for
// both.  Every array lives in the context's scratch arena: the caller holds a CallScope.  The workspace is written by
// apd_round_write with install = 1 only: the x (class 2: and y, z) blocks of u and v.)
struct RoundShared {
    double *rpart = nullptr, *cpart = nullptr;   // a pass's row and column partials; the rest of a side overwrites A's
    double *sA = nullptr, *ab0 = nullptr;        // pass A's scalars; the first marginals [b0 (n); a0 (m)]
};
// what the last kernel of a side leaves on the device for the writing kernels
struct RdDev {
    double theta, t, se, sf;
    long long ok;
};
// what the last kernel of ipd_round_nw.hip leaves for the read-back beside the statistics
struct NwInfoDev {
    long long form, count;        // 0 rank-one, 1 north-west; entries of the list (0 with the rank-one term)
    double cc[2], fval[2];        // mode 2: [0] the rank-one term's, [1] the north-west list's; NaN otherwise
    double pad[2];
};
// a side's arrays of the north-west correction (ipd_round_nw.hip, ipd_round_nw_geo.h); unset under mode 0
struct RoundNw {
    double* pre = nullptr;                               // the prefixes [C_0 .. C_n; R_0 .. R_m]
    int32_t *di = nullptr, *dj = nullptr;                // dense slots: (i, j), i = -1 for an empty slot
    double *dg = nullptr, *dc = nullptr, *dp = nullptr;  // g, c*g, phi*g of a slot
    double *lc = nullptr, *lp = nullptr;                 // c*g, phi*g in list order
    int32_t *li = nullptr, *lj = nullptr;                // the list: the workspace's buffers of this side
    double* lg = nullptr;
    RdDev* devw = nullptr;                               // the writing pass's scalars: t = 0 when the list carries t
    NwInfoDev* info = nullptr;
};
struct RoundSide {
    int side = 0;
    double *sc = nullptr, *ab2 = nullptr, *ef = nullptr;   // [kappa; rho], [b2; a2], [f; e]: n + m entries each
    double *sC = nullptr, *sD = nullptr;                   // the scalars of C and D
    ipd_round_stats* out = nullptr;                        // device, APD_STATS_DOUBLES doubles
    void* dev = nullptr;                                   // what the last kernel leaves for the writing kernels
    RoundNw nw;
};
// tol, install: IPD_E_ARG; finite gama: IPD_E_UNSUPPORTED
void apd_round_check_args(const ipd_apd* h, double tol, int32_t install);
RoundShared apd_round_pass_a(ipd_apd* h, double tol);
// out_dev: where the statistics go, nullptr: into the scratch; info_dev likewise, under a mode other than 0
RoundSide apd_round_first_scale(ipd_apd* h, const RoundShared& sh, int side, ipd_round_stats* out_dev,
                                NwInfoDev* info_dev = nullptr);
void apd_round_rest(ipd_apd* h, const RoundShared& sh, const RoundSide& s, double tol);
void apd_round_write(ipd_apd* h, const RoundShared& sh, const RoundSide& s, double tol, int install, double* x_out_dev);

// ---- ipd_round_nw.hip ----------------------------------------------------------------------
// (the north-west-corner correction along the workspace's orders; reached from the stages above
// when h->corr_mode != 0, never under mode 0)
// a side's scratch and its list buffers; info_dev: where the read-back's second part goes, nullptr: into the scratch
RoundNw apd_nw_side(ipd_apd* h, int side, NwInfoDev* info_dev);
// after k_rd_fin<2> (mode 2: and after pass D): scans, merge and the last kernel; s.out, s.dev, s.nw.devw and
// s.nw.info are complete on the stream afterwards
void apd_nw_rest(ipd_apd* h, const RoundShared& sh, const RoundSide& s);
// after pass W wrote theta*X2: t*g added at the list's entries of up to three destinations
void apd_nw_scatter(ipd_apd* h, const RoundSide& s, int need_ok, double* o0, double* o1, double* o2);
// what a finished call used becomes what ipd_apd_correction_entries and ipd_apd_correction_info return; info = nullptr:
// the rank-one term of mode 0
void apd_nw_record(ipd_apd* h, int side, const NwInfoDev* info);

// ---- ipd_bracket.hip -----------------------------------------------------------------------
// Both certificates of the state in one pass over what they share (ipd_apd_bracket).  The caller
// holds a CallScope: lam and the sides' arrays live in the scratch arena.
struct BracketRun {
    ipd_bracket b;           // read back and picked on the host
    double tol = 0.0;
    const double* lam[2] = {nullptr, nullptr};   // the two repaired multipliers (L entries each)
    RoundShared shared;
    RoundSide side[2];
};
// everything up to the one read-back and the two picks; the workspace is only read
BracketRun apd_bracket_measure(ipd_apd* h, double tol);
// the rounded plan of r.b.upper_side becomes the state; r.b.upper.ok must be 1
void apd_bracket_install(ipd_apd* h, const BracketRun& r);
