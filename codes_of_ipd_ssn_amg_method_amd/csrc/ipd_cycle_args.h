// Descriptors and kernel-argument records of the cycle's kernels that the host side keeps in its state
// (ipd_cycle_state.h): what the host fills and the kernels read.  No kernel, so that a host unit can name a record
// without compiling its kernel (the phases' records come with their inline device code: ipd_cycle_phases.h).
#pragma once

#include "ipd_cycle_dev.h"      // LevelDev
#include "ipd_cycle_phases.h"   // SmoothArgs, XferArgs, TopArgs
#include "ipd_limits.h"

// hist[0] = res0 (set on the first call), hist[1] = res, hist[2] = previous res,
// hist[3] = rel_res, hist[4] = rhok                        Class_AMG.m:89,103-105
struct ConvArgs {
    const double* r;
    int n;
    double* hist;
    int first;
};

// ---------------------------------------------------------------------------
// PCG (Shewchuk B3) in one workgroup                              PCG.m:68-87
// ---------------------------------------------------------------------------
// The hot use is the coarsest level (N <= 1+fix(M^(1/3)), i.e. <= 17 rows): the
// whole solve is latency, so it runs inside one workgroup with no host round
// trips.  Vectors live in global scratch (L1/L2 resident).  precd: 1 none, 2 Jacobi.
struct PcgArgs {
    int N, L;
    const int* rp;
    const int* ci;
    const double* va;
    const double* rhs;
    const double* guess;  // NULL -> zeros
    double* d;            // solution
    double* work;         // 4*N doubles: r, p, q, diag
    double tol;
    long long maxit;
    int precd;
    double* out;          // out[0] = it, out[1] = res ; then resk[0..min(it,nresk))
    long long nresk;
};

// The fused single-workgroup program (k_fused): a list of phase descriptors that travels as kernel arguments
struct ResidDesc {
    LevelDev lv;
    const double* e;
    int row0, row1;
};
enum : int { PH_SMOOTH = 1, PH_RESID, PH_XFER, PH_TOP, PH_PCG, PH_CONV };
struct PhaseDesc {
    int type;
    int pad_;
    union U {
        SmoothArgs s;
        ResidDesc r;
        XferArgs x;
        TopArgs t;
        PcgArgs p;
        ConvArgs c;
    } u;
};
static constexpr int FUSED_MAX = 16;
struct FusedProg {
    int n;
    int pad_;
    PhaseDesc d[FUSED_MAX];
};
static_assert(sizeof(FusedProg) <= 3900, "fused program must fit the 4 KiB kernel-argument segment");

// ---------------------------------------------------------------------------
// matrix-free level-1 operator (the ASAtz.m idea, made to work)
// ---------------------------------------------------------------------------
// In Hybrid_AMG's rescaled system Ae = bk1*Q0^2 + (Q0*T*Q0 + Q0*H0*Q0)/tk the off-diagonal
// block is the active-set mask times a rank-one matrix: Ae(j, n+i) = -s_ij * (q_j^2/tk) * p_i^2.
// A Gauss-Seidel half sweep on the bipartite level therefore needs ONE BIT per entry plus
// two scale vectors instead of 12 bytes: at rho = 1, m = n = 1024 a half sweep reads 128 KB of
// mask instead of 12.6 MB of CSR.  The operator is derived from A_1's own CSR arrays and is
// used only if every entry matches the rank-one form to 1e-12 (k_maskop_build verifies), so a
// caller that hands in any other matrix silently keeps the CSR kernels.
struct MaskOp {
    int nf, nc;           // F rows (column constraints, n), C rows (row constraints, m)
    int nwf, nwc;         // 64-bit words per F row (over i) and per C row (over j)
    const unsigned long long* fbits;  // [nf][nwf]
    const unsigned long long* cbits;  // [nc][nwc]
    const double* alpha;  // nf: q_j^2 / tk
    const double* beta;   // nc: p_i^2
    const double* diag;   // nf + nc
};

// ---------------------------------------------------------------------------
// whole Class_AMG solve phase in ONE workgroup
// ---------------------------------------------------------------------------
// Realistic Newton systems have tiny hierarchies (every level a few thousand nonzeros,
// SURVEY F4/F5): a W cycle is then several hundred dependent micro-phases and the
// multi-launch path is bound by launch latency and by the host (measured 1.9 ms per
// W cycle at M = 1000).  Here one workgroup interprets the V/W recursion itself
// (MG_Vcycle.m:12-45, MG_Wcycle.m:13-46), the stationary iteration and its stopping
// rules (Class_AMG.m:86-109): one launch and one read-back per solve.
struct SolveLevel {
    LevelDev lv;
    double* e;
    double* e2;
    double* w;
    XferArgs rest;  // r_{k+1} = P' rr_k      (valid for k < J)
    XferArgs prol;  // e_k += P e_{k+1}
    int nnzA, nnzP;  // sizes for the LDS cache copy
    // tiny levels (<= 32 rows) also carry DENSE column-major copies in LDS: M[i + j*rows].
    // Their operators are 50-90 % full, and a dense row walk has affine, independent LDS
    // addresses (no index -> value dependency), which is what a single wave needs to pipeline.
    const double* dA;   // N x N
    const double* dP;   // N x Nc   (prolongation, k < J)
    const double* dPt;  // Nc x N   (restriction,  k < J)
    // One-wave levels in POLYNOMIAL form (k_pack_poly, see tiny_cycle): the nu sweeps of a visit are
    // one fixed linear map, e' = S^nu e + (I + S + ... + S^(nu-1)) Rg r, so the level carries the
    // stacked dense operators below instead of dA / dP / dPt and a visit is two passes.  NULL: sweeps.
    // Layout: column-major with a fixed leading dimension pLD in {32, 48, 64} >= N + Nc and the column
    // count padded to a multiple of 8 with zero columns (the vectors of these levels are zero-padded
    // likewise): every load of a pass then has a compile-time offset from one base address.
    // pMr, pMe, pMc lie one behind the other in the image (a pass streams through them).
    const double* pMr;  // [M2a; P' - (P'A) M2a]  applied to r          (M2 = M2a + w 1': see k_pack_poly)
    const double* pMe;  // [M1; -(P'A) M1]        applied to the iterate (kept start, post-smoothing)
    const double* pMc;  // M1 P                   applied to the child's correction
    const double* pW;   // [w; -(P'A) w]          times 1'r
    int pLD;
    // Thread-per-row levels: lane map (k_pack_lmap, see blk_sweeps) -- BT words {row | sub << 10 |
    // log2(lanes of the row) << 14 | valid << 31} and one word "entries per lane" (0: walk in a loop).
    const unsigned* lmap;
    // Small, nearly full thread-per-row levels (level 4 of the early Newton systems: 60-100 rows, 50-100 %
    // full): the image carries the dense copy dA instead of the CSR arrays, and a lane keeps its part of
    // the row (columns sub, sub + Lr, ...) in registers for the visit (blk_sweeps).
    int blk_dense;
    // Thread-per-row levels of 49..144 rows in BLOCK-WIDE polynomial form (k_bpoly_*, see bpoly_pass):
    // the same stacked operators as pMr / pMe / pMc, [Mr | Me | Mc] one behind the other, column-major
    // with gLD in {128, 256} rows, in GLOBAL memory (they do not fit in LDS: 200-500 KB; the tail's
    // compute unit streams them from L2 twice per visit).  NULL: sweeps.
    const double* gM;
    const double* gW;
    int gLD;
};
struct SolveDesc {
    int J, nu, isnsp, wcycle, anycycle, maxit;
    int k_lds;        // levels k_lds..J (and the transfers between them) are cached in LDS
    int k_tiny;       // levels k_tiny..J have <= 32 rows: their whole sub-cycle runs in ONE wave
    int k_blk;        // cached Jacobi levels k_blk..k_tiny-1: one thread per row (blk_cycle)
    int k_semi;       // 0, or a sub-cycle root whose vectors sit in LDS while its matrix, its
                      // transfers and its constant vectors are read from global memory (L2)
    // LDS image: this descriptor, a relocation table and the constant arrays of the cached
    // levels are laid out in global memory exactly as they will sit in LDS (behind the staging
    // area); pointers into the image are stored as LDS byte offsets and relocated on arrival
    int image_bytes;  // multiple of 16; 0 = nothing cached
    int lds_total;    // dynamic LDS the kernel is launched with: staging area, image, work vectors
    int dbg_skip;     // timing by elimination (IPD_DEBUG_SKIP=<mask>, results are then garbage): 1 the
                      // polynomial passes skip their streams, 2 the coarsest PCG does no iteration, 4 the
                      // thread-per-row sweeps skip the row walk, 8 no sweeps at all on those levels
    int nreloc;
    double* root_r;   // k_subcycle: global right-hand side / correction of the root level
    double* root_e;
    long long* dbg;   // optional: wall_clock64 stamps (100 MHz) of k_subcycle's stages
    int stage_bytes;  // size of the gather staging area at the start of dynamic LDS
    double* bp_part;  // LDS: 8 x gLD partial sums + 8 (block-wide polynomial passes)
    // One block-wide polynomial level's operator as an LDS copy (round 4): a compact column-major copy of
    // L[bm_level].gM with bm_ld rows (the stacked N + Nc <= 128, rounded up to even) sits at bm_src; a kernel whose
    // launch carries lds_total + bm_bytes of dynamic LDS (the resident kernels' tail workgroup, which serves a whole
    // solve out of one image load) copies it to LDS offset bm_off and its passes read it there -- 0.7 us per pass
    // against 1.7 us out of L2.  bm_bytes = 0: none.
    const double* bm_src;
    int bm_level, bm_ld, bm_off, bm_bytes;
    double retol;
    PcgArgs pcg;
    SolveLevel L[SOLVE_ML + 1];
};
