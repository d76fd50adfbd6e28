// Device-resident AMG hierarchy: the reference's `global Ack Prok J smoth_it Rk`
// (AMG/Class_AMG.m:42-47) as one handle.
#pragma once

#include "ipd_internal.h"
#include "ipd_launch_plan.h"   // HalfRanges

// Filled-in amg_options (Class_AMG.m:26-34 defaults applied).
struct AmgOpts {
    double retol = 1e-12;
    int bigph = 0;
    int maxit = 50;
    double theta = 0.25;
    int smoth = 3;
    int cycle = 'v';
    int isnsp = 0;
    int inter = 1;
    long long fnode = -1;
    // AMG/twogrid_bigph.m as a special case of the hierarchy: exactly two levels whatever the
    // size (:25-38), coarse solve PCG(Ac, rrc, struct('retol',[],'maxit',1e2,'precd',2)) (:72-73)
    bool twogrid = false;
    long long pcg_maxit = 10000;   // MG_Vcycle.m:43 PCG(A,r): PCG.m:20 defaults
    // AMG4POT's two solves run side by side (Class2/AMG4POT.m:46-47): at most one of them finds the compute units
    // for a resident kernel of 200+ workgroups, the other runs as launches -- the planner then keeps the LDS
    // image the launches do best with (rooted at level 4) instead of the one the resident kernel does best with
    bool concurrent_pair = false;
    // Hybrid_AMG / AMG4POT / the drivers with AMG-PCG as the inner solver (ipd_hybrid_amg_pcg,
    // ipd_amg4pot_pcg, ipd_apd_set_krylov): every Class_AMG solve phase (Hybrid_AMG.m:41, :70) is
    // amg_pcg_planned_dev from the same random guess with this retol and maxit; setup, components,
    // small blocks and the rand stream are untouched.  Not an amg_options field.
    bool krylov = false;
};
AmgOpts amg_fill_twogrid_defaults(const ipd_amg_opts* o);
AmgOpts amg_fill_defaults(const ipd_amg_opts* o);

struct Level {
    int N = 0;          // rows of A
    Csr A;              // Ack{k}
    Csr P;              // Prok{k}   : N_{k-1} x N_k   (k >= 2; stored on the coarse level)
    Csr Pt;             // Prok{k}'  : N_k x N_{k-1}   (restriction, CSR)
    Csr T1;             // Prok{k}'*A_{k-1} : the first product of the Galerkin triple (transfer.m:66),
                        // kept for the fused residual + restriction  r_k = P'r - (P'A) e
    uint8_t* cmask = nullptr;  // isC of level k-1 (N_{k-1} bytes), k >= 2
    // smoother Rk{k}: level 1 with bigph -> forward Gauss-Seidel on the [F|C] blocks
    // (dinv = 1/diag, nf = fnode); otherwise weighted Jacobi (dinv = 0.5/diag, nf = 0)
    double* dinv = nullptr;
    int nf = 0;
    double* Axi = nullptr;  // A*1   (MG_Vcycle.m:15)
    double* xx = nullptr;   // device scalar 1'*A*1
    // work vectors of the cycle
    double* r = nullptr;    // right-hand side of this level
    double* e = nullptr;    // iterate
    double* e2 = nullptr;   // ping-pong partner of e
    double* w = nullptr;    // first-half result of a Gauss-Seidel sweep (without the +c shift)
    double* rr = nullptr;   // residual r - A e
    double* scal = nullptr; // small device scalars (sum r, partial dots ...)
};

struct CycleState;   // ipd_cycle_state.h
struct KrylovState;  // ipd_krylov.hip
struct BlockState;   // ipd_block_state.h
struct BlockKrylovState;   // ipd_block_krylov.hip
struct LevelDev;     // ipd_cycle_dev.h

struct ipd_amg {
    ipd_ctx* ctx = nullptr;
    std::shared_ptr<CycleState> cyc;  // launch geometry + partial-sum buffers
    std::unique_ptr<Arena> arena;
    // Hierarchy whose rand-independent part this one shares (levels 1 and 2 of a bigraph
    // hierarchy: A_1, its smoother data and padded copy, P_2, P_2', A_2 -- the level-1 transfer
    // draws no random numbers, AMG/transfer.m:19-25): constant device arrays are pointed at, not
    // copied; work vectors and everything from level 2's C/F split down are this hierarchy's own.
    std::shared_ptr<ipd_amg> donor;
    AmgOpts opts;
    int J = 0;
    std::vector<Level> L;  // 1-based like the MATLAB cells; L[0] unused
    // solve-phase buffers (level-1 sized)
    double* x = nullptr;
    double* b = nullptr;
    double* res = nullptr;   // A x - b
    double* hist = nullptr;  // device copy of [res0, res, rnorm]
    // PCG work vectors for the coarsest level
    double* pcg_work = nullptr;
    // AMG-preconditioned CG (ipd_krylov.hip): its level-1 sized vectors, scalars and tickets out of
    // `arena`, made on the first ipd_amg_pcg call
    std::shared_ptr<KrylovState> kry;
    // block solve of several right-hand sides (ipd_block.hip, block_state): its N x W work blocks out of
    // `arena`, made on the first ipd_amg_solve_multi or ipd_amg_pcg_multi call and made again for a wider W
    std::shared_ptr<BlockState> blk;
    // AMG-PCG of several right-hand sides (ipd_block_krylov.hip): its N x W vectors, scalars and tickets
    // out of `arena`, made on the first ipd_amg_pcg_multi call and made again for a wider W
    std::shared_ptr<BlockKrylovState> bkry;
};

// ipd_coarsen.hip, ipd_setup.hip (what they call each other through: ipd_setup_internal.h)
void amg_strength_mask(ipd_ctx* ctx, const Csr& A, double theta, uint8_t* strong, int* degi,
                       int* rowcnt);
void amg_mis_set(ipd_ctx* ctx, const Csr& A, double theta, ipd_rng* rng, uint8_t* isC,
                 uint8_t* isF, uint8_t* strong_out /*nnz bytes or NULL*/);
void amg_transfer(ipd_ctx* ctx, Arena& dst, const Csr& A, const AmgOpts& o, int level,
                  ipd_rng* rng, Csr* Ac, Csr* P, Csr* Pt, uint8_t* cmask /*A.nr bytes*/,
                  Csr* T1out = nullptr /* Pt*A kept in dst when asked for */);
ipd_amg* amg_setup(ipd_ctx* ctx, const Csr& A, const AmgOpts& o, ipd_rng* rng,
                   const std::shared_ptr<ipd_amg>& donor = nullptr);
int amg_coarsest_threshold(int N);

// ipd_cycle.hip (amg_attach_maskop: ipd_resident_host.hip; amg_pcg_small_ok, amg_pcg_small_launch: ipd_small.hip)
void amg_prepare_levels(ipd_amg* h);  // dinv, Axi, xx, work vectors
void amg_cycle(ipd_amg* h, int k, int isnsp, bool wcycle, bool keep_e);
bool amg_attach_maskop(ipd_amg* h, const double* p_dev, const double* q_dev, int m, int n, double tk,
                       bool policy, bool transfers_only = false);
void amg_solve_dev(ipd_amg* h, const double* b_dev, const double* guess_dev, double* x_dev,
                   int32_t* it, double* rel_res, double* rel_resk, double* rhok);
// Level 1's launch-path row walk (descriptor, LDS staging, grid of a whole-level pass); false when
// the level is sharded over ranks.  amg_apply_cycle: L[1].e = one cycle from zero on L[1].r with
// the hierarchy's own cycle and isnsp (IPD_E_ARG for a cycle other than 'v'/'w'), queue flushed.
bool amg_level1_walk(ipd_amg* h, LevelDev* lv, int* staged, int* grid);
void amg_apply_cycle(ipd_amg* h);
// The whole AMG-PCG solve as ONE single-workgroup launch (k_pcg_small) on a hierarchy planned for the
// single-workgroup solve (amg_pcg_small_ok: an IMG_SOLVE image, not sharded).  The launch is queued on
// h->ctx's stream; the caller reads `out` back: out[0] = it, out[1] = res, out[2] = delta_0, resk at
// out[4 .. 4 + maxit).  d holds the initial guess going in and the solution coming out.
struct PcgSmallVecs {
    const double* e = nullptr;
    double* d = nullptr;
    double* r = nullptr;
    double* p = nullptr;
    double* q = nullptr;
    double* w_old = nullptr;
    double* out = nullptr;     // 4 + maxit doubles
};
bool amg_pcg_small_ok(ipd_amg* h);
void amg_pcg_small_launch(ipd_amg* h, const PcgSmallVecs& v, double tol, int maxit);
// ipd_krylov.hip: [d,it,res,resk] = AMG_PCG(h,e,pcg_options) on device vectors, as one launch where the
// hierarchy is planned for it and as launches elsewhere (resk: host, maxit slots or NULL)
void amg_pcg_planned_dev(ipd_amg* h, const double* e, const double* guess, double tol, long long maxit,
                         double* d_out, long long* it_out, double* res_out, double* resk);
// What the block cycle (ipd_block.hip; BlockState: ipd_block_state.h) needs of a level's launch-path cycle: the CSR matrices with
// their lanes per row and whole-level grids, the smoother data and the coarsest PCG's settings.
struct BlockCsr {
    int nr = 0, nc = 0;
    int L = 1, grid = 1;       // lanes per row, workgroups of a whole-matrix row walk
    const int* rp = nullptr;   // NULL: absent
    const int* ci = nullptr;
    const double* va = nullptr;
};
struct BlockLevel {
    int N = 0, nf = 0;                  // rows, F-block size (0: Jacobi)
    BlockCsr A;
    HalfRanges sweep[2];                // pre, post: the row ranges of a smoother sweep and their grids
    const double* dinv = nullptr;
    const double* Axi = nullptr;
    const double* xx = nullptr;
    BlockCsr Pt, P, T1;                 // k < J: restriction, prolongation; T1 = P'A when the fused
                                        // residual + restriction applies (else T1.rp == NULL)
    int pcg_L = 1, pcg_precd = 2;       // k == J: PCG(A,r) of the cycle
    double pcg_tol = 0.0;
    long long pcg_maxit = 0;
};
// 1-based levels (out[0] unused; out == NULL: the check alone); false when the hierarchy runs sharded
// over ranks
bool amg_block_levels(ipd_amg* h, std::vector<BlockLevel>* out);
void pcg_dev(ipd_ctx* ctx, const Csr& H, const double* e, const double* guess, double tol,
             long long maxit, int precd, double* d, long long* it, double* res, double* resk_host,
             long long nf = 0);

// ipd_dense.hip: dense Cholesky (MATLAB's `\` on the cold paths' SPD systems)
void dense_chol_factor(ipd_ctx* ctx, double* A, int n, int ld);              // lower triangle, in place
void dense_chol_solve(ipd_ctx* ctx, const double* L, int n, int ld, double* B, int nrhs, int ldb);
void spd_solve_dev(ipd_ctx* ctx, const Csr& A, const double* b, double* x);  // x = A \ b
