/*
 * ipd_amg.h -- C ABI of libipdamg, the MI355X-native (gfx950, hand-written HIP)
 * implementation of the AMG V/W-cycle solve and the ASAt KKT assembly of
 * zihang-student/Codes-of-IPD-SsN-AMG-method.
 *
 * The reference has no FFI layer: its boundary is the MATLAB function
 * signature set itself.  Each entry point below names the
 * MATLAB signature (reference file:line) it replaces; the MEX gateway that a
 * maintainer adds on the reference side is `codes_of_ipd_ssn_amg_method_amd/
 * mex/ipd_mex.cpp`, described in INTEGRATION.md.
 *
 * Conventions
 *  - every function returns 0 on success, a negative IPD_E_* code on failure;
 *    ipd_last_error() returns the thread-local message of the last failure
 *    (the MEX shim forwards it through mexErrMsgIdAndTxt, mirroring MATLAB's
 *    error()).
 *  - sparse matrices cross the boundary in MATLAB's own layout: compressed
 *    sparse column, 0-based int64 indices (binary compatible with mwIndex),
 *    float64 values, row indices ascending, no explicit zeros.
 *  - dense vectors are float64, matrices column-major; logical vectors are one
 *    byte per entry (mxLogical).
 *  - the caller owns every input buffer; nothing is retained after the call
 *    except by an explicit handle (ipd_amg, ipd_dmat).  Output matrices are
 *    library-owned host buffers released with ipd_csc_free().
 *  - pointers are HOST pointers unless the function name ends in `_dev`.
 *  - all arithmetic is IEEE float64; there is no CPU fallback: every entry
 *    point fails with IPD_E_HIP when no gfx950 device is usable.
 */
#ifndef IPD_AMG_H
#define IPD_AMG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPD_VERSION 100 /* 0.1.0 */

enum {
    IPD_OK = 0,
    IPD_E_ARG = -1,      /* bad argument (the reference's error() guards)    */
    IPD_E_HIP = -2,      /* HIP runtime failure / no device                  */
    IPD_E_NOMEM = -3,
    IPD_E_LIMIT = -4,    /* size above a documented library limit            */
    IPD_E_NUMERIC = -5,  /* e.g. coarsening stalled, zero pivot              */
    IPD_E_UNSUPPORTED = -6,
    IPD_E_COMM = -7      /* RCCL failure                                     */
};

typedef struct ipd_ctx ipd_ctx;   /* one per process+GPU: device, stream, workspace   */
typedef struct ipd_rng ipd_rng;   /* MATLAB-compatible rand stream (mt19937ar)        */
typedef struct ipd_amg ipd_amg;   /* device-resident hierarchy: Ack, Prok, Rk, J      */
typedef struct ipd_dmat ipd_dmat; /* device-resident sparse matrix (CSR, int32+fp64)  */

/* Host view of a MATLAB sparse matrix (read-only input). */
typedef struct ipd_csc {
    int64_t nrows, ncols, nnz;
    const int64_t* jc; /* ncols+1 column pointers */
    const int64_t* ir; /* nnz row indices         */
    const double* pr;  /* nnz values              */
} ipd_csc;

/* Library-owned output matrix (same layout); release with ipd_csc_free. */
typedef struct ipd_csc_out {
    int64_t nrows, ncols, nnz;
    int64_t* jc;
    int64_t* ir;
    double* pr;
} ipd_csc_out;

/* amg_options struct (Class1/APD_SsN_Class1.m:87-88, AMG/Class_AMG.m:20-34).
 * Unset numeric fields use the sentinel -1 ("isempty" in MATLAB) and receive
 * Class_AMG's empty-field defaults. */
typedef struct ipd_amg_opts {
    double retol;   /* default 1e-12 */
    int32_t bigph;  /* default 0     */
    int32_t maxit;  /* default 50    */
    double theta;   /* default 1/4   */
    int32_t smoth;  /* default 3     */
    int32_t cycle;  /* 'v' or 'w' (ASCII); default 'v'; any other value: no correction (quirk A-8) */
    int32_t isnsp;  /* default 0     */
    int32_t inter;  /* default 1 (ignored for inter<2, transfer.m:54 quirk)  */
    int64_t fnode;  /* required >0 when bigph                                */
} ipd_amg_opts;

/* pcg_options struct (PCG.m:18-27). */
typedef struct ipd_pcg_opts {
    double retol;   /* default 1e-11 */
    int64_t maxit;  /* default 10000 */
    int32_t precd;  /* 1 none, 2 Jacobi, 3 SSOR (w = 1.5), 4 ichol(H) with MATLAB's defaults
                       (IC(0), PCG.m:46), 5 SSOR on the bigraph blocks              */
    int64_t nf;     /* precd 5: size of the F block (pcg_options.nf, PCG.m:55)      */
} ipd_pcg_opts;

/* prob_data struct (Class1/APD_SsN_Class1.m:154-156, Class2/APD_SsN_Class2.m:163-166). */
typedef struct ipd_prob {
    int64_t m, n;      /* length(p), length(q)                                */
    double bk1, tk;
    const double* p;   /* m */
    const double* q;   /* n */
    const double* t;   /* diag(T), n+m entries, or NULL for T = 0             */
    const ipd_csc* H0; /* (n+m) x (n+m), output of ASAt                       */
    const double* z;   /* n+m  (n+m+1 for AMG4POT)                            */
    const uint8_t* s;  /* m*n logical, AMG4POT only                           */
    const double* phi; /* m*n, AMG4POT only                                   */
} ipd_prob;

/* ---- library / context -------------------------------------------------- */
int ipd_version(void);
const char* ipd_last_error(void);
/* Number of HIP devices this process sees (hipGetDeviceCount); 0 without a usable GPU.  bench.py's
 * ranks map LOCAL_RANK onto it before a context exists.                                          */
int ipd_device_count(int32_t* count);
int ipd_ctx_create(int device, ipd_ctx** out);
void ipd_ctx_destroy(ipd_ctx* ctx);
int ipd_ctx_sync(ipd_ctx* ctx);
void ipd_csc_free(ipd_csc_out* mat);
void ipd_amg_opts_init(ipd_amg_opts* o); /* all fields "empty"               */
void ipd_pcg_opts_init(ipd_pcg_opts* o);

/* ---- rand stream (Hybrid_AMG.m:40,69; AMG/mis_set.m:31,35) --------------- */
/* mt19937ar seeded like MATLAB rng(seed); seed 5489 == MATLAB's default.    */
int ipd_rng_create(uint32_t seed, ipd_rng** out);
/* replays caller-supplied doubles (e.g. MATLAB's own rand output); running
 * out of numbers is IPD_E_ARG.                                              */
int ipd_rng_create_replay(const double* values, int64_t count, ipd_rng** out);
void ipd_rng_destroy(ipd_rng* rng);
int ipd_rng_rand(ipd_rng* rng, int64_t count, double* out); /* rand(count,1) */
int64_t ipd_rng_consumed(const ipd_rng* rng);

/* ---- L0/L1: matrix-free A operators and KKT assembly --------------------- */
/* y = Ax(x,p,q)            Ax.m:2    ; y has n+m entries                     */
int ipd_ax(ipd_ctx*, const double* x, const double* p, const double* q,
           int64_t m, int64_t n, double* y);
/* z = Aty(y,p,q)           Aty.m:2   ; z has m*n entries                     */
int ipd_aty(ipd_ctx*, const double* y, const double* p, const double* q,
            int64_t m, int64_t n, double* z);
/* H = ASAt(s,p,q)          ASAt.m:2                                          */
int ipd_asat(ipd_ctx*, const uint8_t* s, const double* p, const double* q,
             int64_t m, int64_t n, ipd_csc_out* H);
/* y = invAAt(x,p,q,sg1,sg2) invAAt.m:1 (nargin handling is the shim's job)   */
int ipd_inv_aat(ipd_ctx*, const double* x, const double* p, const double* q,
                int64_t m, int64_t n, double sg1, double sg2, double* y);
/* y = invHHt(v,p,q,sg,phi)  Class2/invHHt.m:1 ; v,y have n+m+1 entries       */
int ipd_inv_hht(ipd_ctx*, const double* v, const double* p, const double* q,
                int64_t m, int64_t n, double sg, const double* phi, double* y);

/* ---- L2: AMG setup pieces ------------------------------------------------ */
/* S = strength(A,which)    AMG/strength.m:1                                  */
int ipd_strength(ipd_ctx*, const ipd_csc* A, int which, ipd_csc_out* S);
/* [indC,indF] = cf_split(S) AMG/cf_split.m:1 (SubG is rebuilt by the shim)   */
int ipd_cf_split(ipd_ctx*, const ipd_csc* S, uint8_t* indC, uint8_t* indF);
/* [isC,isF,As] = mis_set(A,theta)  AMG/mis_set.m:1 ; As may be NULL          */
int ipd_mis_set(ipd_ctx*, const ipd_csc* A, double theta, ipd_rng* rng,
                uint8_t* isC, uint8_t* isF, ipd_csc_out* As);
/* [Ac,Pro] = transfer(A,amg_options) AMG/transfer.m:1 ; level = global J     */
int ipd_transfer(ipd_ctx*, const ipd_csc* A, const ipd_amg_opts* o, int level,
                 ipd_rng* rng, ipd_csc_out* Ac, ipd_csc_out* Pro, uint8_t* indC);

/* ---- L3: hierarchy, cycles, PCG ----------------------------------------- */
/* setup phase of Class_AMG (AMG/Class_AMG.m:41-85); A symmetric              */
int ipd_amg_setup(ipd_ctx*, const ipd_csc* A, const ipd_amg_opts* o, ipd_rng* rng,
                  ipd_amg** out);
void ipd_amg_destroy(ipd_amg* h);
int ipd_amg_num_levels(const ipd_amg* h);                       /* J          */
int ipd_amg_level_dims(const ipd_amg* h, int k, int64_t* rows, int64_t* nnz);
/* download Ack{k} (k>=1), Prok{k} (k>=2), C-mask of level k-1 -> k (k>=2)    */
int ipd_amg_get_A(const ipd_amg* h, int k, ipd_csc_out* A);
int ipd_amg_get_P(const ipd_amg* h, int k, ipd_csc_out* P);
int ipd_amg_get_cmask(const ipd_amg* h, int k, uint8_t* isC /* rows of level k-1 */);
/* solve phase of Class_AMG (AMG/Class_AMG.m:86-109).  rel_resk/rhok need
 * maxit+1 entries (may be NULL); *it = number of cycles.                     */
int ipd_amg_solve(ipd_amg* h, const double* b, const double* guess, double* x,
                  int32_t* it, double* rel_res, double* rel_resk, double* rhok);
/* Several right-hand sides: column j of B (N x nrhs, column-major, leading dimension ldb >= N) goes
 * through the solve phase of Class_AMG (AMG/Class_AMG.m:86-109) on this hierarchy as if it were solved
 * alone -- guess column j (guess may be NULL: zeros), its own count it[j], rel_res[j] and histories
 * (column j of rel_resk / rhok, (maxit+1) x nrhs column-major, each may be NULL; the first it[j]+1
 * entries follow ipd_amg_solve's convention, later slots are left untouched).  A column whose loop
 * has stopped stays frozen while the others go on.  Results agree with ipd_amg_solve to rounding (the
 * summation order differs); they do not depend on the other columns of the call and repeat bit for
 * bit.  Columns run in blocks of up to 8 (the next power of two), chunk by chunk, through block
 * forms of the launch-path cycle: the CSR matrices of every level; an attached mask operator or
 * level-2 polynomial form is ignored.  X (ld = ldb) may not alias B.  IPD_E_ARG for NULL h, B, X or
 * it, nrhs < 1, ldb < N, and a hierarchy set up for a sharded run.
 * For ONE right-hand side ipd_amg_solve stays the call to use: its hierarchies may run the whole
 * solve as one single-workgroup or resident launch.                                              */
int ipd_amg_solve_multi(ipd_amg* h, const double* B, int64_t ldb, int64_t nrhs,
                        const double* guess /* N x nrhs, ld = ldb, or NULL */, double* X /* ld = ldb */,
                        int32_t* it /* nrhs */, double* rel_res /* nrhs or NULL */,
                        double* rel_resk /* (maxit+1) x nrhs or NULL */, double* rhok /* same or NULL */);
/* [d,it,res,resk] = AMG_PCG(h,e,pcg_options): conjugate gradients on level 1 of the hierarchy,
 * preconditioned by one cycle of it from a zero guess -- MG_Vcycle(r,isnsp,1) / MG_Wcycle(r,isnsp,1)
 * with the hierarchy's own cycle, smoth, isnsp, bigph and fnode, the operator ipd_amg_vcycle /
 * ipd_amg_wcycle(h,r,isnsp,1,NULL,e) apply.  The loop is PCG.m:68-87 with one departure: the
 * flexible (Polak-Ribiere) beta = (r'w - r'w_old)/delta_old instead of delta_new/delta_old, since
 * the cycle is not symmetric for isnsp = 1 and its coarsest solve is not linear (both agree for a
 * symmetric linear preconditioner).  pcg_options: retol (default 1e-11) and maxit (default 1e4);
 * precd must stay unset (-1), else IPD_E_ARG; a hierarchy whose cycle is neither 'v' nor 'w' is
 * IPD_E_ARG.  guess may be NULL (zeros); resk needs maxit slots or NULL; e = 0 (with a zero guess)
 * gives it = 0, res = NaN.  Always the launch-path cycle: the resident whole-solve kernels are not
 * used.                                                                                          */
int ipd_amg_pcg(ipd_amg* h, const double* e, const double* guess, const ipd_pcg_opts* o,
                double* d, int64_t* it, double* res, double* resk /* maxit slots or NULL */);
/* ipd_amg_pcg's signature and conventions (precd unset, cycle 'v' / 'w', guess may be NULL, resk of
 * maxit slots or NULL, e = 0 with a zero guess: it = 0, res = NaN), planned like ipd_amg_solve: on a
 * hierarchy planned for the single-workgroup whole solve (every level small, not sharded -- mode 1
 * of ipd_amg_resident_levels) the whole loop, its cycles included, is ONE single-workgroup launch and one
 * read-back.  The cycle is then the single-workgroup kernel's (the same operator as the launch-path
 * cycle, summed in another order), so results agree with ipd_amg_pcg to rounding and repeat bit for
 * bit.  On every other hierarchy, and for maxit above 1000 (a launch stays bounded), it IS
 * ipd_amg_pcg, bit for bit.                                                                      */
int ipd_amg_pcg_planned(ipd_amg* h, const double* e, const double* guess, const ipd_pcg_opts* o,
                        double* d, int64_t* it, double* res, double* resk /* maxit slots or NULL */);
/* How the most recent ipd_amg_pcg / ipd_amg_pcg_planned call (host or _dev) on this hierarchy ran:
 * -1 none yet, 0 as launches, 1 as one single-workgroup launch.                                  */
int ipd_amg_pcg_mode(const ipd_amg* h, int32_t* mode);
/* Several right-hand sides: column j of E (N x nrhs, column-major, leading dimension lde >= N) runs
 * ipd_amg_pcg's loop on this hierarchy as if it were solved alone -- guess column j (guess may be NULL:
 * zeros), its own it[j], res[j] and resk(1:it[j], j) (resk: maxit x nrhs column-major or NULL; later
 * slots are left untouched).  A column that has stopped stays frozen (its D and residual are left
 * alone, its cycle input is zero) while the others go on.  pcg_options, the stop test and the edge
 * conventions are ipd_amg_pcg's (a zero column with a zero guess: it = 0, res = NaN).  Results do not
 * depend on the other columns of the call and repeat bit for bit; they agree with ipd_amg_pcg to
 * rounding (the block cycle sums over the CSR arrays in another order).  Columns run in blocks of up
 * to 8 (the next power of two), chunk by chunk, through block forms of the launch-path cycle, as in
 * ipd_amg_solve_multi: an attached mask operator or level-2 polynomial form is ignored.  D (ld = lde)
 * may not alias E; rows N..lde-1 of D are the caller's and are carried through.  IPD_E_ARG for NULL
 * h, E, D or it, nrhs < 1, lde < N, precd set, a cycle other than 'v' / 'w', and a hierarchy set up
 * for a sharded run.                                                                             */
int ipd_amg_pcg_multi(ipd_amg* h, const double* E, int64_t lde, int64_t nrhs,
                      const double* guess /* N x nrhs, ld = lde, or NULL */, const ipd_pcg_opts* o,
                      double* D /* ld = lde */, int64_t* it /* nrhs */, double* res /* nrhs or NULL */,
                      double* resk /* maxit x nrhs or NULL */);
/* e = MG_Vcycle(r,isnsp,k)   AMG/MG_Vcycle.m:2 ; k is 1-based               */
int ipd_amg_vcycle(ipd_amg* h, const double* r, int isnsp, int k, double* e);
/* e = MG_Wcycle(r,isnsp,k,e) AMG/MG_Wcycle.m:2 ; e_inout NULL-able input    */
int ipd_amg_wcycle(ipd_amg* h, const double* r, int isnsp, int k,
                   const double* e_in, double* e_out);
/* [x,it,rel_res,rel_resk,rhok] = Class_AMG(A,b,amg_options) Class_AMG.m:1   */
int ipd_class_amg(ipd_ctx*, const ipd_csc* A, const double* b, const double* guess,
                  const ipd_amg_opts* o, ipd_rng* rng, double* x, int32_t* it,
                  double* rel_res, double* rel_resk, double* rhok);
/* [x,it,rel_res,rel_resk,rhok] = twogrid_bigph(A,b,amg_options) AMG/twogrid_bigph.m:1:
 * the two-level special case (exactly one coarse level, coarse PCG with maxit 100); empty
 * fields take twogrid_bigph.m:11-15's defaults (retol 0, maxit 50, smoth 3, isnsp 0);
 * amg_options.fnode is required.  rel_resk/rhok need maxit+1 slots.                     */
int ipd_twogrid_bigph(ipd_ctx*, const ipd_csc* A, const double* b, const double* guess,
                      const ipd_amg_opts* o, double* x, int32_t* it, double* rel_res,
                      double* rel_resk, double* rhok);
/* [x,it,rel_res,rel_resk,rhok] = twogrid(A,b,amg_options) AMG/twogrid.m:1: bigph = 0 (default)
 * smooths with .5*D^-1 and coarsens with mis_set(A,1/4) (needs `rng`); bigph = 1 as above    */
int ipd_twogrid(ipd_ctx*, const ipd_csc* A, const double* b, const double* guess,
                const ipd_amg_opts* o, ipd_rng* rng, double* x, int32_t* it, double* rel_res,
                double* rel_resk, double* rhok);
/* [d,it,res,resk] = PCG(H,e,pcg_options)   PCG.m:1 ; resk needs maxit slots
 * or NULL                                                                    */
int ipd_pcg(ipd_ctx*, const ipd_csc* H, const double* e, const double* guess,
            const ipd_pcg_opts* o, double* d, int64_t* it, double* res, double* resk);

/* ---- L4: problem-level solvers ------------------------------------------ */
/* [blocks,sizes,p,r] = components(A)  components.m:1 ; 0-based outputs,
 * components numbered by smallest member (dmperm's order is unpinned).       */
int ipd_components(ipd_ctx*, const ipd_csc* A, int64_t* blocks, int64_t* sizes,
                   int64_t* p, int64_t* r, int64_t* ncomp);
/* Replays a recorded visiting order of the components (components.m:35-39 takes it from
 * dmperm, whose order is undocumented; Hybrid_AMG.m:55-57 visits in that order, which fixes
 * info(2) and the order in which rand is consumed): smallest_members[k] = the smallest member
 * (0-based) of the component to visit k-th, i.e. min(ps(rs(k):rs(k+1)-1))-1 of a MATLAB
 * recording.  One-shot: applies to the next components / Hybrid_AMG / AMG4POT (and variants)
 * call on this context.  NULL clears it.  Members stay ascending inside a component.        */
int ipd_ctx_set_component_order(ipd_ctx*, const int64_t* smallest_members, int64_t ncomp);
/* [zeta,itamg,resamg,info] = Hybrid_AMG(prob_data,amg_options) Hybrid_AMG.m:1 */
int ipd_hybrid_amg(ipd_ctx*, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                   double* zeta, int32_t* itamg, double* resamg, int64_t info[2]);
/* [zeta,...] = AMG4POT(prob_data,amg_options,'amg')  Class2/AMG4POT.m:1       */
/* [zeta,itpcg,respcg,info] = aug_PCG(prob_data,pcg_options) aug_PCG.m:1 and
 * PCG4POT(prob_data,pcg_options) Class2/PCG4POT.m:1 (inner_solver = 3): Jacobi-PCG on the
 * system augmented with one kernel vector per connected component                          */
int ipd_aug_pcg(ipd_ctx*, const ipd_prob* pd, const ipd_pcg_opts* o, double* zeta,
                int64_t* itpcg, double* respcg, int64_t info[2]);
int ipd_pcg4pot(ipd_ctx*, const ipd_prob* pd, const ipd_pcg_opts* o, double* zeta,
                int64_t* itpcg, double* respcg, int64_t info[2]);
/* [zeta,itamg,resamg,info] = Hybrid_twogrid(prob_data,amg_options) Hybrid_twogrid.m:1 and
 * AMG4POT(prob_data,amg_options,'twogrid') Class2/AMG4POT.m:48-51 (inner_solver = 5)       */
int ipd_hybrid_twogrid(ipd_ctx*, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                       double* zeta, int32_t* itamg, double* resamg, int64_t info[2]);
int ipd_amg4pot_twogrid(ipd_ctx*, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                        double* zeta, int32_t* itamg, double* resamg, int64_t info[2]);
int ipd_amg4pot(ipd_ctx*, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                double* zeta, int32_t* itamg, double* resamg, int64_t info[2]);
/* Hybrid_AMG.m / AMG4POT.m with AMG-preconditioned CG as the inner solver: every Class_AMG call
 * (Hybrid_AMG.m:41, :70) is its setup followed by ipd_amg_pcg_planned from the SAME random guess
 * bk1*tk*rand(size(f)) -- same Ae, f, components, isnsp / fnode rule and small-block direct solves,
 * and the rand stream advances exactly as in Hybrid_AMG.  retol and maxit are amg_options' (Class_AMG's
 * defaults when unset); itamg = the most PCG iterations over the large components, resamg = their
 * largest PCG res, info as in Hybrid_AMG.  The mask form of level 1 is not attached: the PCG's level-1
 * product and its cycle walk A_1's rows.                                                          */
int ipd_hybrid_amg_pcg(ipd_ctx*, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                       double* zeta, int32_t* itamg, double* resamg, int64_t info[2]);
int ipd_amg4pot_pcg(ipd_ctx*, const ipd_prob* pd, const ipd_amg_opts* o, ipd_rng* rng,
                    double* zeta, int32_t* itamg, double* resamg, int64_t info[2]);

/* ---- device-resident path (inputs already in HBM) ------------------------ */
/* A device pointer needs only the alignment of its element type (8 bytes for double, 1 for a mask
 * byte): a slice of a larger array is a valid argument.  Wider accesses are taken where the address
 * allows them and give the same result.                                                        */
/* raw device memory on the context's GPU */
int ipd_dmalloc(ipd_ctx*, size_t bytes, void** dptr);
int ipd_dfree(ipd_ctx*, void* dptr);
int ipd_h2d(ipd_ctx*, void* dst_dev, const void* src_host, size_t bytes);
int ipd_d2h(ipd_ctx*, void* dst_host, const void* src_dev, size_t bytes);
/* device matrices */
int ipd_dmat_upload(ipd_ctx*, const ipd_csc* A, int symmetric, ipd_dmat** out);
int ipd_dmat_download(ipd_ctx*, const ipd_dmat* A, ipd_csc_out* out);
int ipd_dmat_dims(const ipd_dmat* A, int64_t* rows, int64_t* cols, int64_t* nnz);
void ipd_dmat_destroy(ipd_dmat* A);
/* C = A*B for sparse operands, every C(i,j) summed in ascending inner index with separately
 * rounded multiply and add -- the order of MATLAB's sparse mtimes as `Pro'*A*Pro`
 * (AMG/transfer.m:66) uses it; exact zeros are dropped from the result                      */
int ipd_dmat_multiply(ipd_ctx*, const ipd_dmat* A, const ipd_dmat* B, ipd_dmat** out);
/* y = A*x on device vectors (CSR row walk)                                   */
int ipd_spmv_dev(ipd_ctx*, const ipd_dmat* A, const double* x_dev, double* y_dev);
int ipd_ax_dev(ipd_ctx*, const double* x_dev, const double* p_dev, const double* q_dev,
               int64_t m, int64_t n, double* y_dev);
int ipd_aty_dev(ipd_ctx*, const double* y_dev, const double* p_dev, const double* q_dev,
                int64_t m, int64_t n, double* z_dev);
int ipd_asat_dev(ipd_ctx*, const uint8_t* s_dev, const double* p_dev, const double* q_dev,
                 int64_t m, int64_t n, ipd_dmat** H);
/* The hierarchy keeps its own copy of A: the ipd_dmat may be destroyed as soon as the call returns. */
int ipd_amg_setup_dev(ipd_ctx*, const ipd_dmat* A, const ipd_amg_opts* o, ipd_rng* rng,
                      ipd_amg** out);
int ipd_amg_solve_dev(ipd_amg* h, const double* b_dev, const double* guess_dev,
                      double* x_dev, int32_t* it, double* rel_res, double* rel_resk,
                      double* rhok);
/* ipd_amg_solve_multi on device blocks B, guess (or NULL) and X; it, rel_res and the histories stay
 * host arrays                                                                                    */
int ipd_amg_solve_multi_dev(ipd_amg* h, const double* B_dev, int64_t ldb, int64_t nrhs,
                            const double* guess_dev, double* X_dev, int32_t* it, double* rel_res,
                            double* rel_resk, double* rhok);
/* ipd_amg_pcg on device vectors (guess_dev may be NULL); resk stays a host array               */
int ipd_amg_pcg_dev(ipd_amg* h, const double* e_dev, const double* guess_dev,
                    const ipd_pcg_opts* o, double* d_dev, int64_t* it, double* res, double* resk);
/* ipd_amg_pcg_planned on device vectors (guess_dev may be NULL); resk stays a host array       */
int ipd_amg_pcg_planned_dev(ipd_amg* h, const double* e_dev, const double* guess_dev,
                            const ipd_pcg_opts* o, double* d_dev, int64_t* it, double* res, double* resk);
/* ipd_amg_pcg_multi on device blocks E, guess (or NULL) and D; it, res and resk stay host arrays */
int ipd_amg_pcg_multi_dev(ipd_amg* h, const double* E_dev, int64_t lde, int64_t nrhs,
                          const double* guess_dev, const ipd_pcg_opts* o, double* D_dev, int64_t* it,
                          double* res, double* resk);
/* Hybrid_AMG with H0 already on the device (output of ipd_asat_dev)          */
int ipd_hybrid_amg_dev(ipd_ctx*, const ipd_dmat* H0, const double* t_dev, const double* p_dev,
                       const double* q_dev, int64_t m, int64_t n, double bk1, double tk,
                       const double* z_dev, const ipd_amg_opts* o, ipd_rng* rng,
                       double* zeta_dev, int32_t* itamg, double* resamg, int64_t info[2]);
/* ipd_hybrid_amg_pcg with H0 already on the device                          */
int ipd_hybrid_amg_pcg_dev(ipd_ctx*, const ipd_dmat* H0, const double* t_dev, const double* p_dev,
                           const double* q_dev, int64_t m, int64_t n, double bk1, double tk,
                           const double* z_dev, const ipd_amg_opts* o, ipd_rng* rng,
                           double* zeta_dev, int32_t* itamg, double* resamg, int64_t info[2]);

/* X = A \ B, MATLAB's mldivide for a sparse symmetric positive definite A (CSC, both triangles)
 * and a dense column-major B (n x nrhs): the reference's cold-path direct solves
 * `zeta = Jk \ (-Fk_old)` (Class1/APD_SsN_Class1.m:148, Class2/APD_SsN_Class2.m:155) and
 * `W = -Aff \ Afc` (AMG/transfer.m:58).  MATLAB uses CHOLMOD (closed source); this is a blocked
 * dense Cholesky on the device, n <= 16384.  IPD_E_NUMERIC when A is not positive definite.     */
int ipd_spd_solve(ipd_ctx*, const ipd_csc* A, const double* B, int64_t nrhs, double* X);

/* ---- L5: APD / semismooth-Newton drivers and A-ADMM warm starts ----------- */
/* SURVEY.md section 8 rows f1/f2.  The reference's drivers are MATLAB *scripts*
 * (Class1/APD_SsN_Class1.m, Class2/APD_SsN_Class2.m): their boundary is the
 * workspace they load (`c,r,l,p,q,gama` resp. `C,r,l,p,q,mu,phi`) and the
 * variables they leave behind (`xk, lk, fxk, KKT_xk, KKT_lk, SsN_itnum,
 * PCG_itnum, SumAMG, ...`).  `ipd_apd` holds that workspace in HBM; every mn-
 * sized vector stays on the device for the whole run.                        */
typedef struct ipd_apd ipd_apd;

typedef struct ipd_apd_data {
    int32_t cls;          /* 1 = transport-like (Class 1), 2 = partial OT (Class 2)   */
    int64_t m, n;
    const double* c;      /* mn, column-major cost                                     */
    const double* r;      /* n                                                         */
    const double* l;      /* m                                                         */
    const double* p;      /* m                                                         */
    const double* q;      /* n                                                         */
    const double* gama;   /* class 1: mn upper bounds, or NULL -> gama_scalar          */
    double gama_scalar;   /* class 1: scalar bound, +Inf allowed (data1-*.mat)         */
    double mu;            /* class 2: transported mass                                 */
    const double* phi;    /* class 2: mn                                               */
} ipd_apd_data;

/* Script constants (APD_SsN_Class1.m:35-36, APD_SsN_Class2.m:35-36).          */
typedef struct ipd_apd_opts {
    int32_t maxit;        /* 100                                                       */
    double kkt_tol;       /* 1e-6                                                      */
    int32_t ssn_it;       /* 50                                                        */
    double ssn_tol1;      /* class 1: 1e-11, class 2: 1e-10                            */
    double nu, delta;     /* 0.2, 0.9                                                  */
    int32_t ll_max;       /* 500                                                       */
    int32_t prob;         /* class 1 only: `prob` of :19-23; 3 selects the merit of :186 */
    int32_t inner_solver; /* :66-71: 4 AMG (default), 5 two-grid, 3 aug_PCG / PCG4POT,
                             2 plain PCG on Jk, 1 direct solve `Jk \ (-Fk_old)`           */
    double pcg_retol;     /* pcg_options of :81,84: 1e-11                               */
    int64_t pcg_maxit;    /*                        1e4                                 */
} ipd_apd_opts;
void ipd_apd_opts_init(int32_t cls, ipd_apd_opts* o);

/* One record per Newton step: what the reference prints with format `cc`/`bb`
 * (APD_SsN_Class1.m:91-92,215-236) plus the size of the active set.            */
typedef struct ipd_ssn_rec {
    int32_t k, ssn_it, ll, itamg;
    int64_t E, info0, info1;
    double Fk_norm, resamg, bk1, tk;
} ipd_ssn_rec;

typedef struct ipd_apd_result {
    int32_t converged;    /* `CONV at it = k`                                          */
    int32_t k;            /* APD iterations done so far                                */
    double fval;          /* fxk(k+1) = c'*xk                                          */
    double kkt[4];        /* KKT_xk, KKT_lk, KKT_yk, KKT_zk of the last iterate        */
    double rr;            /* max relative KKT residual (:265)                          */
    int64_t sum_amg, total_amg, fail_amg, max_amg;   /* SumAMG ... MaxAMG (:94-97)     */
    int32_t restarts;
    int64_t nrec;         /* Newton-step records available through ipd_apd_records     */
} ipd_apd_result;

int ipd_apd_create(ipd_ctx*, const ipd_apd_data* d, ipd_apd** out);
void ipd_apd_destroy(ipd_apd* h);
/* lengths of uk (mn, or mn+n+m for class 2) and lk (n+m, or n+m+1)                 */
int ipd_apd_dims(const ipd_apd* h, int64_t* len_u, int64_t* len_lam);
/* [xk,lk] = warmup_class1(c,r,l,p,q,gama,res,maxit) (Class1/warmup_class1.m:2) and
 * [uk,lk] = warmup_class2(c,r,l,p,q,mu,phi,res,maxit) (Class2/warmup_class2.m:1):
 * the result becomes the driver state (xk = vk = xk0, lk = lk0, bk = 1; Class1 :59-60).
 * maxit < 0 means `inf`; the nargin/res rules of :3-20 are applied.              */
int ipd_apd_warmup(ipd_apd* h, double res, int64_t maxit);
/* Workspace access.  u = xk (mn) for class 1, uk = [xk;yk;zk] (mn+n+m) for class 2;
 * lam = lk (n+m resp. n+m+1).  NULL pointers are skipped.                        */
int ipd_apd_set_state(ipd_apd* h, const double* u, const double* v, const double* lam, double bk);
int ipd_apd_get_state(ipd_apd* h, double* u, double* v, double* lam, double* bk);
/* on != 0: inner_solver = 4 runs ipd_hybrid_amg_pcg resp. ipd_amg4pot_pcg instead of Hybrid_AMG /
 * AMG4POT 'amg'; FailAMG / MaxAMG / TotalAMG / SumAMG and the per-step records then count PCG
 * iterations by the same rules (itamg == amg_options.maxit is a failure).  Off (the default) is
 * the stationary iteration; other inner solvers ignore it.  Holds until changed.                 */
int ipd_apd_set_krylov(ipd_apd* h, int32_t on);
/* Runs up to `iters` further APD iterations (`for k = 1:maxit`, Class1 :101-275,
 * Class2 :95-285) with inner_solver = 4 (Hybrid_AMG resp. AMG4POT 'amg'); stops
 * early at `CONV` or at opts->maxit.                                              */
int ipd_apd_run(ipd_apd* h, const ipd_apd_opts* o, const ipd_amg_opts* amg, ipd_rng* rng,
                int32_t iters, ipd_apd_result* res);
/* Histories: which = 0 fxk, 1 KKT_xk, 2 KKT_lk, 3 KKT_yk, 4 KKT_zk (k+1 entries),
 * 5 SsN_itnum (k entries).  Returns the number of entries written in *count.    */
int ipd_apd_history(const ipd_apd* h, int32_t which, double* out, int64_t cap, int64_t* count);
int ipd_apd_records(const ipd_apd* h, ipd_ssn_rec* out, int64_t cap, int64_t* count);
/* Row f3 of SURVEY.md section 8 (hierarchy reuse across Newton steps).  The reference sets the
 * hierarchy up at every Newton step (Hybrid_AMG.m:40-41, AMG/Class_AMG.m:41-85); when a step's
 * system equals the previous step's (same active set, T, bk1, tk) its setups share the previous
 * hierarchies' rand-independent levels 1-2, bit for bit the same result (IPD_NO_STEP_DONOR=1
 * rebuilds everything).  *steps = Newton steps solved with AMG, *same_system = those whose system
 * repeated, *donated = setups that took levels from the previous step.  NULLs are skipped.    */
int ipd_apd_reuse_stats(const ipd_apd* h, int64_t* steps, int64_t* same_system, int64_t* donated);
/* Building blocks of one APD iteration, exposed for parity tests and callers that
 * keep the outer loop: `begin` fixes k and forms ak, bk1, tk, wk, wlk (:113-126);
 * `eval` evaluates zk = (wk - H'*lam)/tk, s, Fk = bk1*lam - H*prox(zk) - wlk and the
 * line-search merit cFk (:139-144,182-196) in ONE pass over wk.
 * vals = {bk1, tk, ak, |Fk|, cFk, E}.                                            */
int ipd_apd_begin(ipd_apd* h, int32_t k, double vals[3]);
int ipd_apd_eval(ipd_apd* h, const double* lam, uint8_t* s_out, double* t_out, double* Fk_out,
                 double vals[6]);
/* The other blocks of an iteration, for the same two uses.  All need `begin` first (except `end`
 * with from_w = 0); vectors are host arrays, lam / zeta / Fk of ipd_apd_dims' len_lam entries,
 * u / wk of len_u; NULL outputs are skipped.
 * `get_w`: wk and wlk as `begin` left them.
 * `eval_trial`: `eval` at the line search's trial point lam + step*zeta (:189,200; zeta NULL: at
 *   lam), as apd's Newton loop calls it: lam_out is the multiplier the pass used, Fk_old (with
 *   zeta; may be NULL) gives fold_zeta = Fk_old'*zeta (:198), merit3 != 0 (class 1) takes the
 *   prob-3 merit |zk|^2 - |zk - prox(zk)|^2 (:183-187), whose sums z2, zmp2 are 0 otherwise.
 *   vals = {bk1, tk, ak, |Fk|, cFk, E, z2, zmp2, fold_zeta, lam2, wlk_lam, prox2}; the last
 *   three are the raw sums |lam|^2, wlk'*lam, |prox(zk)|^2 that cFk is made of.
 * `merit`: cFk at lam + steps[k]*zeta for the IPD_APD_MERIT_STEPS trial steps one pass of the
 *   line search takes together (:199-207).
 * `end`: from_w != 0 forms uk1 = prox(zk) and vk1 at the multiplier lam (:239-242) -- u must be
 *   NULL -- and makes (uk1, vk1, lam) the state ipd_apd_get_state reads, as an iteration
 *   without a restart does; from_w = 0 measures the iterate u (NULL: the state's) at lam and
 *   changes nothing.  kkt = {KKT_xk, KKT_lk, KKT_yk, KKT_zk}, *fx = c'*x.                      */
#define IPD_APD_MERIT_STEPS 8
int ipd_apd_get_w(ipd_apd* h, double* wk, double* wlk);
int ipd_apd_eval_trial(ipd_apd* h, const double* lam, const double* zeta, double step,
                       const double* Fk_old, int32_t merit3, uint8_t* s_out, double* t_out,
                       double* Fk_out, double* lam_out, double vals[12]);
int ipd_apd_merit(ipd_apd* h, const double* lam, const double* zeta,
                  const double steps[IPD_APD_MERIT_STEPS], double merit[IPD_APD_MERIT_STEPS]);
int ipd_apd_end(ipd_apd* h, int32_t from_w, const double* lam, const double* u, double kkt[4],
                double* fx);
/* HIP-event timing of `reps` eval passes on the current workspace (bench.py).   */
int ipd_apd_bench_eval(ipd_apd* h, int32_t reps, double* total_ms, double* bytes_per_pass);

/* The transport plan as a sparse matrix, out of and into the device workspace:
 * the dense iterate stays in HBM, only the kept entries and n+1 column pointers cross.          */
typedef struct ipd_plan_stats {
    int64_t nnz;         /* entries kept                                         */
    double sum_kept;     /* sum of x over kept entries                           */
    double sum_dropped;  /* sum of |x| over dropped entries                      */
    double max_dropped;  /* largest |x| dropped, 0 if none                       */
    double fval_kept;    /* sum of c.*x over kept entries                        */
} ipd_plan_stats;

/* X = sparse(reshape(xk,m,n)) restricted to entries with !(|x| <= tol): m x n CSC, rows ascending in
 * every column, library-owned (ipd_csc_free).  xk is the first mn entries of the workspace's u
 * (class 2: the x block of uk).  tol = 0 is exactly MATLAB's sparse(): nonzeros and NaNs are kept.
 * ax (n+m, or NULL) receives Ax(x_kept,p,q) = [X'*p ; X*q].  IPD_E_ARG for NULL h, X or st, and
 * for tol negative or NaN.                                                                       */
int ipd_apd_plan(ipd_apd* h, double tol, ipd_csc_out* X, ipd_plan_stats* st, double* ax);

/* Same, into caller-owned DEVICE arrays: jc_dev n+1, ir_dev / pr_dev cap entries.  *st is filled in
 * either case; when st->nnz > cap only jc_dev is written and the call returns IPD_E_LIMIT (so a
 * first call with cap = 0 is the size query; ir_dev / pr_dev may then be NULL).  ax_dev: n+m or
 * NULL.  IPD_E_ARG for NULL h, st or jc_dev, cap < 0, tol negative or NaN.                       */
int ipd_apd_plan_dev(ipd_apd* h, double tol, int64_t cap, int64_t* jc_dev, int64_t* ir_dev,
                     double* pr_dev, ipd_plan_stats* st, double* ax_dev);

/* xk = vk = full(X) (Class1 :60); class 2: the x blocks of uk and vk, the y and z blocks untouched.
 * lk, bk, histories and records are left exactly as ipd_apd_set_state(u, v, NULL, bk_unchanged)
 * with the dense equivalent would leave them.  X is validated on the host before anything is
 * uploaded: IPD_E_ARG (state unchanged) for dimensions other than m x n, jc[0] != 0, jc not
 * non-decreasing, jc[n] != nnz, a row index outside [0, m), rows not strictly ascending within a
 * column.                                                                                        */
int ipd_apd_set_plan(ipd_apd* h, const ipd_csc* X);

/* The plan applied on the device: with X what ipd_apd_plan returns at this tol (a NaN is
 * kept, tol = 0 keeps every nonzero; class 2: the x block of uk),
 *   side = 0:  Y = X*B,   B n x k as B[j + c*n],  Y m x k as Y[i + c*m],  w = X*1  (m entries)
 *   side = 1:  Y = X'*B,  B m x k as B[i + c*m],  Y n x k as Y[j + c*n],  w = X'*1 (n entries)
 * -- the layouts of ipd_cost_spec::xs / ys, so a point cloud goes in as it is.  k is in [1, 16]; w may be
 * NULL and is the plain mass of the kept entries (p and q are not applied: that is ax of ipd_apd_plan).
 * A dropped entry contributes exactly +0.0 whatever B holds there: an inf or NaN in a row of B that meets
 * only dropped entries does not reach Y (B is not checked for finiteness otherwise).  normalize = 1
 * divides row r of Y by w[r], one IEEE division per entry (the barycentric projection when B is a point
 * cloud); a row of zero kept mass is 0/0 = NaN.  Deterministic: two calls, and the two entries, give the
 * same bits.  The workspace is only read -- state, script variables, histories and partial buffers are as
 * before -- and neither c nor the coordinates are touched, so stored, point-cloud and matrix-free
 * workspaces behave alike.  IPD_E_ARG for a NULL h, B or Y, side or normalize outside {0, 1}, tol negative
 * or NaN; IPD_E_LIMIT for k outside [1, 16]; nothing is written then.  Both return when the result is
 * complete.                                                                                         */
int ipd_apd_plan_apply(ipd_apd* h, double tol, int32_t side, int32_t k, int32_t normalize,
                       const double* B, double* Y, double* w);          /* host arrays   */
int ipd_apd_plan_apply_dev(ipd_apd* h, double tol, int32_t side, int32_t k, int32_t normalize,
                           const double* B_dev, double* Y_dev, double* w_dev);   /* device arrays */

/* The dual certificate on the device.  With C = reshape(c,m,n), lam = [alpha (n); beta (m)] and,
 * class 2, tau behind them, b = [r; l(; mu)], the reduced cost (Aty.m) is
 *   d(i,j) = ((C(i,j) + p_i*alpha_j) + q_j*beta_i) [+ tau*phi(i,j)],   class 2 also: d_y = alpha, d_z = beta,
 * and the dual value g(lam) = -<b,lam> - sum_ij gama_ij*max(0, -d_ij); for gama = inf and for class 2 the last
 * sum is dropped and lam is feasible when d >= 0 (class 2: over all three blocks).
 *   side = -1  evaluates lam (L entries, NULL: the workspace's lk) as it is.
 *   side =  0  holds alpha and replaces beta by its c-transform, beta^_i = max_j t(i,j) with
 *              t(i,j) = ((-C(i,j) [- tau*phi(i,j)]) - p_i*alpha_j) / q_j, then evaluates the result;
 *   side =  1  holds beta: alpha^_j = max_i ((-C(i,j) [- tau*phi(i,j)]) - q_j*beta_i) / p_i.
 * Class 2 first clamps the held side to max(., 0) and clamps the new side likewise.  Every operation is one IEEE
 * operation in the order written; a NaN candidate counts as -inf; of equal maxima the smallest index wins.  With
 * r, l >= 0 the transform yields the best feasible multiplier for the held side.  lam_out (L entries or NULL)
 * receives the repaired multiplier -- the held side (clamped for class 2), the new side, tau passed through --
 * and arg (NULL, or m entries for side 0, n for side 1) the winning column (row); both are ignored for
 * side = -1.  primal = 1 adds fval = <c, xk> of the workspace's iterate and the gap (the only case that reads u).
 * Deterministic: two calls, and the two entries, give the same bits; stored, point-cloud and matrix-free
 * workspaces give the same bits.  The workspace is only read -- state, script variables, histories and partial
 * buffers are as before; scratch comes from the context's arena.  IPD_E_ARG for a NULL h or st, side outside
 * {-1, 0, 1}, primal outside {0, 1}, and for a transform whose divider (q for side 0, p for side 1) has an
 * entry that is <= 0 or not finite (checked once per workspace and remembered); IPD_E_UNSUPPORTED for
 * side >= 0 on a class-1 workspace with finite gama (every lam is feasible there); nothing is written then.
 * Both return when the result is complete.                                                              */
typedef struct ipd_dual_stats {
    double dual, bterm, cap;     /* g(lam_out); -<b,lam_out>; sum gama*max(0,-d), 0 when dropped             */
    double dmin;                 /* smallest reduced cost of lam_out (class 2: over d, alpha, beta)         */
    int64_t imin, jmin, nneg;    /* first place of dmin in column-major order (-1,-1 if in the y/z blocks);
                                    count of d < 0 (class 2: over all three blocks)                         */
    double fval, gap;            /* <c, xk> of the workspace iterate and fval - dual; NaN when primal = 0   */
} ipd_dual_stats;
int ipd_apd_dual(ipd_apd* h, const double* lam, int32_t side, int32_t primal,
                 double* lam_out, int32_t* arg, ipd_dual_stats* st);          /* host arrays   */
int ipd_apd_dual_dev(ipd_apd* h, const double* lam_dev, int32_t side, int32_t primal,
                     double* lam_out_dev, int32_t* arg_dev, ipd_dual_stats* st);   /* device arrays; st on the host */

/* The primal certificate on the device: the iterate rounded onto the feasible set, and the exact cost
 * of the result -- Altschuler, Weed and Rigollet's Algorithm 2 with the weights p, q and class 2's phi row.  With
 * X = reshape(x,m,n) the x block of the workspace's u, C the cost, PHI class 2's phi, and the constraints of Ax.m
 * (class 1: sum_i p_i X_ij = r_j, sum_j q_j X_ij = l_i; class 2: both with <=, and sum phi_ij X_ij = mu), every
 * operation below one IEEE operation in the order written:
 *    1  clamp        x+_ij = (!(|x_ij| <= tol) && x_ij > 0) ? x_ij : 0     (ipd_apd_plan's threshold, then the clamp
 *                    at 0; a NaN becomes 0)
 *    2  marginals    a0_i = sum_j q_j*x+_ij,   b0_j = sum_i p_i*x+_ij
 *    3  side = 0     rho_i = a0_i > l_i ? l_i/a0_i : 1;   b1_j = sum_i p_i*(rho_i*x+_ij);
 *                    kappa_j = b1_j > r_j ? r_j/b1_j : 1
 *    4  side = 1     kappa_j = b0_j > r_j ? r_j/b0_j : 1;   a1_i = sum_j q_j*(x+_ij*kappa_j);
 *                    rho_i = a1_i > l_i ? l_i/a1_i : 1
 *    5  scaled plan  X2_ij = (rho_i*x+_ij)*kappa_j
 *    6  its sums     a2_i = sum_j q_j*X2_ij,  b2_j = sum_i p_i*X2_ij,  fs = sum c_ij*X2_ij,
 *                    class 2: ms = sum phi_ij*X2_ij
 *    7  deficits     e_i = max(l_i - a2_i, 0),  f_j = max(r_j - b2_j, 0),  the clamp written d > 0 ? d : 0
 *    8  their sums   Se = sum p_i*e_i,  Sf = sum q_j*f_j,  cc = sum c_ij*(e_i*f_j),  class 2: cp = sum phi_ij*(e_i*f_j)
 *    9  class 1      theta = 1,  t = Se > 0 ? 1/Se : 0
 *   10  class 2      ms >= mu:  theta = mu/ms, t = 0;   otherwise  theta = 1, t = (mu - ms)/cp
 *   11  result       X^_ij = theta*X2_ij + t*(e_i*f_j),   fval = theta*fs + t*cc,
 *                    class 2: y^_j = max(r_j - (theta*b2_j + t*(Se*f_j)), 0),  z^_i = max(l_i - (theta*a2_i + t*(e_i*Sf)), 0)
 *   12  ok = 1 iff theta, t and fval are finite and, class 2, t*Se <= 1 and t*Sf <= 1.  ok = 0: no repair of this
 *       shape exists -- a result, not an error.
 * X^ stays factored: rho (m), kappa (n), e (m), f (n) -- each may be NULL -- with theta and t of the statistics
 * rebuild it from x; x_out_dev (mn entries or NULL, not the workspace's own) receives it in full.  viol_in is
 * sum p_i|a0_i - l_i| + sum q_j|b0_j - r_j| (class 2: the positive parts of a0_i - l_i and b0_j - r_j only), dropped
 * the sum of |x| over the nonzero entries that step 1 set to 0 and ndropped their count (a NaN is counted and adds
 * nothing to dropped); ms and cp are NaN for class 1.
 * Summation shapes (fixed: two calls, the two entries, and stored, point-cloud and matrix-free workspaces give the
 * same bits; no float atomics): with column groups of 64 columns and segments of 64 rows, a row sum (a0, a1, a2) adds
 * the columns of a group in ascending order and then the groups in ascending order; a column sum (b0, b1, b2) adds
 * the 64 rows of a segment in the butterfly of the tile walker's colsum16 and then the segments in ascending order; a
 * scalar over mn entries (fs, ms, cc, cp, dropped, ndropped) adds a row's entries of a column group in ascending
 * order, the 64 rows of a segment in a fixed tree, the four segments of a 256-row block in order, and the blocks
 * (column-group major) as entries t, t + 256, ... per thread t, the 256 threads in the same tree; Se, Sf and the two
 * halves of viol_in add entries t, t + 256, ... per thread and then that tree.
 * install = 1 makes X^ the state: the x blocks of u and v are written, class 2 also their y and z blocks with y^ and
 * z^; lk, bk, histories and records are untouched.  It is refused with IPD_E_NUMERIC, state unchanged and nothing
 * written, when ok = 0.  With install = 0 the workspace is only read.  Scratch comes from the context's arena.
 * IPD_E_ARG for a NULL h or st, side or install outside {0, 1}, tol negative or NaN; IPD_E_UNSUPPORTED for a class-1
 * workspace with finite gama, scalar or vector (the rank-one term does not keep x <= gama); nothing is written then.
 * Both return when the result is complete.                                                                      */
typedef struct ipd_round_stats {
    double fval, fs, cc;         /* <c, X^> = theta*fs + t*cc; <c, X2>; sum c_ij*(e_i*f_j)                   */
    double theta, t, se, sf;     /* the scalars of steps 9, 10 and the deficit sums of step 8                */
    double ms, cp;               /* class 2: <phi, X2>, sum phi_ij*(e_i*f_j); NaN for class 1                */
    double viol_in, dropped;     /* weighted marginal violation of x+; sum |x| over entries step 1 zeroed    */
    int64_t ndropped;            /* their count                                                              */
    int32_t ok;
} ipd_round_stats;
int ipd_apd_round(ipd_apd* h, double tol, int32_t side, int32_t install,
                  double* rho, double* kappa, double* e, double* f, ipd_round_stats* st);      /* host arrays */
int ipd_apd_round_dev(ipd_apd* h, double tol, int32_t side, int32_t install,
                      double* rho_dev, double* kappa_dev, double* e_dev, double* f_dev,
                      double* x_out_dev, ipd_round_stats* st);   /* device arrays; st on the host */

/* The rounding's correction: what carries the deficits e, f of step 7 into X^.  A workspace setting,
 * obeyed by ipd_apd_round, ipd_apd_round_dev, ipd_apd_bracket, ipd_apd_bracket_dev and the gap rule's probes.
 *    mode 0  the rank-one term t*(e_i*f_j) of steps 8 and 11 above: the default, and what a workspace without the
 *            setting computes, in the same bits
 *    mode 1  a north-west-corner coupling G of the deficits along a row order sigma and a column order tau
 *    mode 2  both are evaluated and the device keeps the one with ok = 1 first, then the one with the smaller fval
 *            (class 1: the smaller cc, t being the same); the rank-one term stays on a tie
 * Steps 1-7, 9, 10 and 12, Se, Sf and step 11's y^, z^ are as above; G replaces e_i*f_j in cc, cp and X^.  Every
 * operation is one IEEE operation in the order written:
 *   N1  orders      sigma a permutation of 0..m-1, tau of 0..n-1 (host int32 arrays; NULL is the identity)
 *   N2  masses      alpha_k = (p_i*e_i)*Sf, i = sigma_k, k = 1..m;   beta_s = (q_j*f_j)*Se, j = tau_s, s = 1..n
 *                   (both sum to Se*Sf in exact arithmetic)
 *   N3  prefixes    R_0 = C_0 = 0; R_k, C_s the inclusive prefix sums of alpha, beta in this shape: the vector is cut
 *                   into chunks of 64 entries; within a chunk c the local prefixes L are formed by adding its entries
 *                   in ascending order, starting from the chunk's first entry; the chunk offsets are O_0 = 0,
 *                   O_c+1 = O_c + (last local prefix of chunk c), in ascending order; a prefix is O_c + L (chunk 0:
 *                   L itself).  In numpy: L = cumsum(alpha.reshape(-1, 64), axis=1), O = [0, cumsum(L[:, -1])[:-1]],
 *                   R = O[:, None] + L.  The shape depends on nothing but the vector; with non-negative masses the
 *                   prefixes are non-decreasing, across chunk edges too, which N4 relies on.
 *   N4  entries     for every (k, s) with w = min(R_k, C_s) - max(R_k-1, C_s-1) > 0 one entry i = sigma_k, j = tau_s,
 *                   g = w/(p_i*q_j); at most m + n - 1 entries, each (i, j) at most once, listed in ascending (k, s).
 *                   An interval of one vector that lies beyond the other vector's total -- the two totals differ by
 *                   their rounding at most -- has no entry.
 *   N5  marginals   sum_j q_j*G_ij = e_i*Sf and sum_i p_i*G_ij = f_j*Se up to the rounding of N3: the rank-one term's
 *                   marginals, which is why t, ok, y^ and z^ keep their formulas
 *   N6  sums        cc = sum c_ij*g, class 2: cp = sum phi_ij*g, over the list in list order in Se's shape (entries
 *                   t, t + 256, ... per thread t, then the tree)
 *   N7  result      X^_ij = theta*X2_ij, and X^_ij = theta*X2_ij + t*g at the list's entries
 * ipd_round_stats keeps its layout: cc and cp hold the sums of the form that was used.  c_ij is taken from the
 * workspace's cost source, so stored, point-cloud and matrix-free workspaces give the same bits; two calls and the
 * two entries do too.  An installed plan has at most nnz(x+) + m + n - 1 entries.  Finite gama stays
 * IPD_E_UNSUPPORTED in the rounding calls.
 * ipd_apd_set_correction: the orders are checked on the host and kept on the device with a list of m + n entries per
 * side.  IPD_E_ARG for a NULL h, a mode outside {0, 1, 2} or an order that is not a permutation; IPD_E_LIMIT for a
 * mode other than 0 with m or n above 16384; the setting in force stays then.
 * ipd_apd_correction_entries (host arrays) and ipd_apd_correction_entries_dev (device arrays): the list of the last
 * rounding or bracket call (a bracket: of the chosen side) -- *count its length, 0 when that call used the rank-one
 * term, and the first min(cap, *count) entries into i, j, g (each may be NULL).  IPD_E_ARG for a NULL h or count or
 * cap < 0.  ipd_apd_correction_info: the mode of that call, the form it used (0 rank-one, 1 north-west), the count
 * and, under mode 2, cc and fval of both forms ([0] rank-one, [1] north-west; NaN otherwise).                    */
typedef struct ipd_correction_info {
    int32_t mode, form;
    int64_t count;
    double cc[2], fval[2];
} ipd_correction_info;
int ipd_apd_set_correction(ipd_apd* h, int32_t mode, const int32_t* row_order, const int32_t* col_order);
int ipd_apd_correction_entries(ipd_apd* h, int32_t* i, int32_t* j, double* g, int64_t cap, int64_t* count);
int ipd_apd_correction_entries_dev(ipd_apd* h, int32_t* i_dev, int32_t* j_dev, double* g_dev, int64_t cap,
                                   int64_t* count);
int ipd_apd_correction_info(const ipd_apd* h, ipd_correction_info* out);

/* Both certificates of the state in one call: lower <= f* <= upper.  The two c-transforms of the
 * workspace's lk are formed in one walk over c (class 2: and phi), the two repaired multipliers are evaluated in one
 * read of c and x, the rounding's first pass runs once for both sides, and the four statistics come back in one
 * read-back; the host then picks
 *    lower_side = dual1 > dual0 ? 1 : 0
 *    upper_side = (ok1 > ok0 || (ok1 == ok0 && fval1 < fval0)) ? 1 : 0
 * Every field of lower, and lam_out (L entries or NULL), has the bits of ipd_apd_dual(h, NULL, lower_side, 1, ..);
 * every field of upper, and rho (m), kappa (n), e (m), f (n) -- each may be NULL -- those of
 * ipd_apd_round(h, tol, upper_side, 0, ..): per-entry operations and summation shapes are the ones stated there, and
 * the maxima and minima do not depend on an order.  gap = upper.fval - lower.dual, one subtraction.  install = 1 makes
 * the rounded plan of upper_side the state, as ipd_apd_round(.., upper_side, 1, ..) does; with upper.ok = 0 it is
 * refused with IPD_E_NUMERIC and nothing is written.  With install = 0 the workspace is only read.  Two calls, the two
 * entries, and stored, point-cloud and matrix-free workspaces give the same bits.
 * IPD_E_ARG for a NULL h or out, install outside {0, 1}, tol negative or NaN, p or q with an entry that is <= 0 or not
 * finite; IPD_E_UNSUPPORTED for a class-1 workspace with finite gama; nothing is written then.                   */
typedef struct ipd_bracket {
    ipd_dual_stats lower;             /* of the chosen repaired multiplier                                      */
    ipd_round_stats upper;            /* of the chosen rounded plan                                             */
    int32_t lower_side, upper_side;
    double gap;                       /* upper.fval - lower.dual                                                */
} ipd_bracket;
int ipd_apd_bracket(ipd_apd* h, double tol, int32_t install, double* lam_out,
                    double* rho, double* kappa, double* e, double* f, ipd_bracket* out);          /* host arrays */
int ipd_apd_bracket_dev(ipd_apd* h, double tol, int32_t install, double* lam_out_dev,
                        double* rho_dev, double* kappa_dev, double* e_dev, double* f_dev,
                        ipd_bracket* out);                               /* device arrays; out on the host */

/* A stopping rule of ipd_apd_run on the certified gap.  With a rule set, the bracket above is taken
 * of the state an iteration leaves -- a probe -- after iteration k when
 *    converged || (k >= first && (k - first) % every == 0)
 * so a run that converges always ends with a probe of its final state (final = 1).  Per probe, in this order:
 *    best  = lower > best ? lower : best      (from -inf; every probe's dual value bounds f*, whatever the iterate;
 *                                              the multiplier that attains best is kept on the device)
 *    gap   = upper - best
 *    thr   = max(gap_tol, gap_rel*|upper|)    (both 0: probe and record, never stop)
 *    stop  = thr > 0 && upper_ok && gap <= thr    (a NaN never stops)
 * At a stop the loop ends; ipd_apd_result.converged stays the KKT flag, and further ipd_apd_run calls return at once
 * until the rule is set again, which clears the stop and keeps best and the records.  install = 1 makes the rounded
 * plan the state at the probe that stops, and only there; histories, records, lk and bk stay as ipd_apd_round leaves
 * them.  ipd_apd_set_state (a restart of the script) clears the stop, best and the records; the rule holds until it
 * is changed, NULL switches it off (the default).  Without a rule a run is what it was.
 * ipd_apd_set_gap_rule: IPD_E_UNSUPPORTED for a class-1 workspace with finite gama; IPD_E_ARG for p or q with an entry
 * that is <= 0 or not finite, gap_tol, gap_rel or tol negative or NaN, first or every < 1, install outside {0, 1};
 * the rule in force stays then.
 * ipd_apd_gap_records: as ipd_apd_records.  ipd_apd_gap_lam: *best and, into lam (L entries, host, may be NULL), the
 * multiplier that attains it; before the first probe *best = -inf and lam is not written.                        */
typedef struct ipd_gap_rule {
    double gap_tol, gap_rel;
    double tol;                       /* the rounding's threshold                                               */
    int32_t first, every;             /* both >= 1                                                              */
    int32_t install;
} ipd_gap_rule;
typedef struct ipd_gap_rec {
    int32_t k, lower_side, upper_side, upper_ok, stop, final;
    double lower, lower_dmin, best, upper, viol_in, gap;    /* gap = upper - best */
} ipd_gap_rec;
int ipd_apd_set_gap_rule(ipd_apd* h, const ipd_gap_rule* r);
int ipd_apd_gap_records(const ipd_apd* h, ipd_gap_rec* out, int64_t cap, int64_t* count);
int ipd_apd_gap_lam(ipd_apd* h, double* lam, double* best);

/* The cost matrix built on the device from two point clouds: a driver run is created
 * from (m+n)*d coordinates, nothing mn-sized crosses the host boundary.  With t_k = xs(i,k) - ys(j,k)
 * folded in ascending k into an accumulator that starts at +0.0, multiply and add separate:
 *   1  acc + t_k*t_k        2  the correctly rounded sqrt of metric 1
 *   3  acc + |t_k|          4  max(acc, |t_k|)
 * scale = 1 divides every entry by the largest entry of the unscaled matrix (one IEEE division).  */
typedef struct ipd_cost_spec {
    int32_t metric;      /* 1 sq. Euclidean, 2 Euclidean, 3 city block, 4 Chebyshev */
    int32_t dim;         /* d, 1 .. 16                                               */
    int64_t m, n;
    const double* xs;    /* m*d, xs[i + k*m] (host)                                  */
    const double* ys;    /* n*d, ys[j + k*n] (host)                                  */
    int32_t scale;       /* 0 none, 1 divide by the largest entry                    */
} ipd_cost_spec;
typedef struct ipd_cost_stats { double min, max, sum; } ipd_cost_stats;  /* of what is stored */

/* c_dev[i + j*m] (DEVICE, mn doubles) = the cost of spec *s; *st (or NULL) its statistics, the same
 * bits on every call.  The (m+n)*d coordinates are checked on the host before any launch.  IPD_E_ARG
 * for a NULL ctx, s, c_dev, xs or ys, an unknown metric, dim outside [1, 16], a scale other than 0 or
 * 1, a coordinate that is not finite, and, with scale = 1, a largest entry that is 0 or not finite
 * (c_dev is then unspecified); IPD_E_LIMIT for m or n outside [1, 16384].                         */
int ipd_cost_points_dev(ipd_ctx*, const ipd_cost_spec* s, double* c_dev, ipd_cost_stats* st);
/* ipd_apd_create with the cost made from *s: d->c must be NULL, s->m == d->m and s->n == d->n
 * (IPD_E_ARG otherwise, and for everything ipd_cost_points_dev refuses); for class 2 a NULL d->phi
 * is all ones, filled on the device.  Everything else as ipd_apd_create.  After an error *out is
 * untouched and no workspace exists.                                                               */
int ipd_apd_create_points(ipd_ctx*, const ipd_apd_data* d, const ipd_cost_spec* s, ipd_apd** out);
/* The cost of any workspace: c (mn, host, or NULL) and its statistics (or NULL); a workspace made
 * from a host c computes them at the first call.                                                   */
int ipd_apd_get_cost(ipd_apd* h, double* c, ipd_cost_stats* st);

/* Matrix-free cost: ipd_apd_create_points without the mn doubles of c.  The workspace
 * keeps the (m+n)*d coordinates, and every pass that reads c(i,j) recomputes it with the operations
 * that would have stored it, so each result has the bits of the stored workspace's.  Everything as
 * ipd_apd_create_points, and IPD_E_LIMIT for dim > 3 (the row's coordinates are registers; nothing is
 * stored instead).  ipd_apd_get_cost on such a workspace builds the matrix into scratch memory for
 * the call when c is given; its statistics are those of the stored workspace.                      */
int ipd_apd_create_points_free(ipd_ctx*, const ipd_apd_data* d, const ipd_cost_spec* s, ipd_apd** out);
typedef struct ipd_cost_info {
    int32_t form;          /* 0 stored, 1 matrix-free                                             */
    int32_t dim;           /* of the specification; 0 for a workspace from a host matrix          */
    int32_t metric;        /* likewise                                                            */
    int32_t scale;         /* likewise                                                            */
    int64_t device_bytes;  /* kept for the cost: 8*mn stored, 8*(m+n)*dim matrix-free             */
} ipd_cost_info;
int ipd_apd_cost_info(ipd_apd* h, ipd_cost_info* info);

/* The gradient of the transport cost in the point positions, on the device.  With X what
 * ipd_apd_plan returns at this tol (x(i,j) = u[i + j*m], kept when !(|x| <= tol), a NaN is kept; class 2:
 * the x block of uk) and c the cost of two point clouds, the envelope theorem gives at an optimal -- or
 * rounded feasible, ipd_apd_bracket with install = 1 -- plan
 *   side = 0:  G(i,k) = sum_j X_ij * h_k(i,j),     G m x d as G[i + k*m],  w = X*1  (m entries)
 *   side = 1:  G(j,k) = sum_i X_ij * (-h_k(i,j)),  G n x d as G[j + k*n],  w = X'*1 (n entries)
 * -- the layouts of xs / ys -- with h_k = dc(xs_i, ys_j)/dxs(i,k), every step one IEEE operation, multiply
 * and add separate, t_k = xs(i,k) - ys(j,k):
 *   1  h_k = t_k + t_k
 *   2  a = the entry of metric 2 (folded as the cost is, in ascending k); h_k = t_k / a when a > 0, else +0.0
 *   3  h_k = +1.0, -1.0 or +0.0 by the sign of t_k
 *   4  k* = the smallest k with |t_k| equal to the maximum; h_k* = the sign of t_k*, every other h_k = +0.0
 * Where c is not differentiable (2: a == 0; 3: some t_k == 0; 4: the maximum attained by two coordinates, or
 * 0) that is one subgradient; st->kinks counts the kept entries there, st->kept all kept entries.  scale = 1
 * divides h_k by the largest unscaled entry (one division, applied last; st->denom, 1.0 without scale): the
 * normalisation is held constant -- a stop-gradient -- and the divider is returned so that a caller can add the
 * missing term.  A dropped entry contributes exactly +0.0.  The sums have a fixed shape that depends neither on
 * d nor on how the components are split into passes, and use no atomics: two calls, and the two entries, give
 * the same bits; side 0 adds a row's terms in ascending j within a group of 64 columns, then the groups in
 * ascending order, each from +0.0.  c is never read: every form of workspace gives the same bits.
 * s == NULL (xs_dev == ys_dev == NULL; metric, dim and scale are then ignored) takes the specification and the
 * coordinates the workspace was made from (ipd_apd_create_points, ipd_apd_create_points_free); a workspace
 * from a host c has none: IPD_E_ARG.  A given specification may be used with any workspace: s->m, s->n must
 * be the workspace's, dim is 1 .. 16 on every form, everything ipd_cost_points_dev refuses is refused with its
 * code (the device entry cannot look at device coordinates: they must be finite), and with scale = 1 the
 * divider is computed on the device without storing a matrix (one more read-back; IPD_E_ARG when it is 0 or not
 * finite).  IPD_E_ARG also for a NULL h or G, a side other than 0 or 1, tol negative or NaN, exactly one of
 * xs_dev, ys_dev NULL.  After an error nothing of G, w, st is written.  w and st may be NULL.  The workspace
 * is only read; scratch comes from the context's arena.  Both return when the result is complete.        */
typedef struct ipd_grad_stats {
    int64_t kept;     /* kept entries                                                   */
    int64_t kinks;    /* kept entries at which c is not differentiable                  */
    double denom;     /* the divider of scale = 1 (the largest unscaled entry), else 1.0 */
} ipd_grad_stats;
int ipd_apd_point_grad(ipd_apd* h, const ipd_cost_spec* s, double tol, int32_t side,
                       double* G, double* w, ipd_grad_stats* st);             /* host arrays   */
int ipd_apd_point_grad_dev(ipd_apd* h, int32_t metric, int32_t dim, int32_t scale,
                           const double* xs_dev, const double* ys_dev, double tol, int32_t side,
                           double* G_dev, double* w_dev, ipd_grad_stats* st); /* device arrays */

/* Matrix-free level-1 operator.  If level 1 of `h` is exactly Hybrid_AMG's
 * rescaled operator Ae = bk1*Q0^2 + (Q0*T*Q0 + Q0*H0*Q0)/tk for these p, q, tk (checked entry by
 * entry against A_1's CSR values), the level-1 Gauss-Seidel sweeps read one BIT per entry (the
 * active-set mask) instead of 12 bytes.  *attached = 0 leaves the CSR kernels in place.
 * ipd_hybrid_amg(_dev) and ipd_amg4pot attach it themselves.                               */
int ipd_amg_attach_mask_operator(ipd_amg* h, const double* p_dev, const double* q_dev,
                                 int64_t m, int64_t n, double tk, int32_t* attached);
/* The same check, for the level-resident solve kernel only: its level 1 <-> 2 transfers
 * W(j,i) = s_ij*beta_i*rho_j (AMG/transfer.m:19-25 applied to that operator) then read the bit mask
 * too, whatever the size; the sweeps of the launch path keep their CSR rows.  *attached = 0 when the
 * hierarchy does not run in that kernel or P does not have the form.  The solvers do this themselves. */
int ipd_amg_attach_mask_transfers(ipd_amg* h, const double* p_dev, const double* q_dev,
                                  int64_t m, int64_t n, double tk, int32_t* attached);
/* Level 2 of the level-resident kernel in polynomial form, composed over a whole visit: for a three-level
 * hierarchy with a one-row tail and V cycles (the metric's workload) the smoth pre-sweeps, the residual, the
 * restriction, the tail's prolongation and the smoth post-sweeps of a visit of level 2 (AMG/MG_Vcycle.m:14-41
 * with Class_AMG.m:84's Jacobi smoother) are ONE dense affine map of r_2 (and of the tail's PCG result), packed
 * here by smoth dense products on the f64 matrix cores; a V cycle is then 24 chip-wide hand-offs instead of 33.
 * Same linear operator as the sweeps, different association (rounding at the 1e-16 level per pass).  Packing
 * costs about 0.5 ms at 1024 rows: for many cycles on ONE hierarchy, not for a solve of such a system (one or
 * two cycles) -- the solvers never attach it.  *attached = 0: the hierarchy does not run in that kernel form. */
int ipd_amg_attach_level2_poly(ipd_amg* h, int32_t* attached);

/* ---- measurement hooks (bench.py) ---------------------------------------- */
/* Runs `cycles` iterations of the Class_AMG loop body (residual, one V/W
 * cycle, norm) on the fixed hierarchy without convergence exit, timed with HIP
 * events on the context's stream.  Returns total milliseconds and, per cycle,
 * the algorithmic byte count B_V of SURVEY.md section 8d.                     */
int ipd_amg_bench_cycles(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                         double* total_ms, double* bytes_per_cycle);
/* Times `reps` smoother sweeps of level k (1 <= k < J) with HIP events: the
 * per-launch duration of the dominant kernel.  launches_per_sweep is 2 on the
 * bigraph Gauss-Seidel level (F half, C half) and 1 on Jacobi levels.          */
int ipd_amg_bench_sweeps(ipd_amg* h, int k, int reps, double* total_ms,
                         int* launches_per_sweep, double* bytes_per_sweep);
/* Times `reps` launches of the single-workgroup sub-cycle kernel (levels k_sub..J out of
 * LDS) on a zero right-hand side; stamps = 100 MHz clock at start / image loaded / cycle
 * begins / cycle done inside the last launch, then clocks spent in: wave-level sub-cycles,
 * block-level sweeps, residual+restriction, prolongation.  *k_sub = 0: no such kernel.  */
int ipd_amg_bench_subcycle(ipd_amg* h, int reps, double* total_ms, int32_t* k_sub,
                           int64_t stamps[8]);
/* SURVEY 8d byte model of the hierarchy: per-level S(A_k), S(P_k), ...       */
int ipd_amg_cycle_bytes(const ipd_amg* h, double* bytes_per_cycle);
/* How the solve phase of this hierarchy (AMG/Class_AMG.m:86-109) runs: *mode = 0 one launch
 * per phase, 1 the whole solve in one workgroup (small hierarchies), 2 the whole solve in ONE
 * launch of *grid co-resident workgroups that keep levels 1-2 in registers (csrc/ipd_resident.h:
 * three-level hierarchies of the dense regimes, and hierarchies of 4+ levels whose levels >= 3 fit
 * one workgroup's LDS -- then *grid counts that tail workgroup too); *timeouts = launches of mode 2
 * that gave up and were redone in mode 0.                                                      */
int ipd_amg_solve_mode(const ipd_amg* h, int32_t* mode, int32_t* grid, int32_t* timeouts);
/* Mode 2 only: *levels = levels kept by the resident workgroups (2, 3, or 4: the mask-form kernel's deep
 * mode with levels 3 and 4 in polynomial form), *tail_root = level at which the rest starts (levels + 1);
 * zeros otherwise.                                                                                  */
int ipd_amg_resident_levels(const ipd_amg* h, int32_t* levels, int32_t* tail_root);
/* Mode 2 only: name = the kernel instantiation a solve of this hierarchy launches, as a rocprofv3
 * kernel trace spells it ("k_resident<16,16,0>", "k_resident_big<32>"; "" in the other modes; cap =
 * size of the buffer); *handoffs / *cycles = chip-wide hand-offs (tagged-granule exchanges, visits of
 * the remote tail included) and Class_AMG loop bodies (AMG/Class_AMG.m:96-105) of the LAST launch;
 * *mask_transfers != 0: the level 1 <-> 2 transfers run from the active-set bit mask.  Any output
 * pointer but name may be NULL.                                                                    */
int ipd_amg_resident_kernel(const ipd_amg* h, char* name, int32_t cap, int64_t* handoffs,
                            int32_t* cycles, int32_t* mask_transfers);
/* The variant of that kernel the hierarchy's LAST resident launch took: *full != 0 the full-shape form of the
 * composed instantiation (every size and mode of the metric's shape a constant of the kernel; IPD_RES_NO_FULL=1
 * keeps the general form), *diag != 0 the form that holds the stamps and the skip-publish test hook (a launch of
 * ipd_amg_bench_resident / _classes or one on which IPD_RES_DEBUG_SKIP_PUBLISH fires; the kernels that have no
 * production form always).  Zeros before the first launch.  Either pointer may be NULL.            */
int ipd_amg_resident_variant(const ipd_amg* h, int32_t* full, int32_t* diag);
/* forms[k], k < count (level k = 1..J; forms[0] = 0): how level k runs where it is held in a single
 * workgroup's LDS image (bit mask over the images packed for this hierarchy; 64 / 128: level 3-4 / level 2 of a
 * resident kernel in polynomial form, held by the resident workgroups): 1 thread-per-row sweeps,
 * 2 the same with dense rows in registers, 4 one-wave sweeps, 8 one-wave polynomial form (the nu sweeps,
 * residual and transfers of a visit as two dense passes), 16 block-wide polynomial form (49..144 rows,
 * operators streamed from L2); 0: in no image (launches or the resident workgroups' registers).      */
int ipd_amg_level_forms(const ipd_amg* h, int32_t* forms, int32_t count);
/* Test hook: the block-wide polynomial operator of level k (forms bit 16) as packed for the images:
 * column-major with *ld rows, columns [Mr (N8) | Me (N8) | Mc (Nc8)] and then the column W, N8 / Nc8 =
 * *n / *nc rounded up to 8; `out` needs ld * (2 N8 + Nc8 + 1) doubles (cap = its size).  Rows < n:
 * e' = Mr r + Me e (+ Mc e_c in the second pass) + W 1'r; rows n .. n + nc - 1: the restricted residual
 * (AMG/MG_Vcycle.m:14-41 as two dense maps).  IPD_E_ARG without such an operator. */
int ipd_amg_poly_operator(const ipd_amg* h, int32_t k, double* out, int64_t cap, int32_t* ld, int32_t* n,
                          int32_t* nc);
/* Test hook: the polynomial operator of level k exactly as packed for `form` (ipd_amg_level_forms' bits):
 * 16: the images' column-major layout of ipd_amg_poly_operator (*seg = *n rounded up to 8);
 * 64: level 3 or 4 of a resident kernel (k_resident's `three` mode or the mask-form kernel's deep mode);
 * 128: level 2 composed over a visit (ipd_amg_attach_level2_poly).
 * 64 / 128: row-major, *n + *nc rows of *ld doubles, then the *n + *nc factors of 1'r; `out` needs
 * (*n + *nc) (*ld + 1) doubles.  Row i < n: [M2a | M1 | M1 P] at columns 0, *seg, 2 *seg, factor w_i;
 * row n + c: [P' - T1 M2a | -T1 M1] and factor -T1 w (T1 = P'A).  Form 128 replaces M1 in rows i < n by
 * B = (I + M1) M2a and w_i by (I + M1) w.  out = NULL with cap = 0: only the layout (*ld, *seg, *n, *nc).
 * IPD_E_ARG when level k has no operator in that form, or cap is below what the layout needs.       */
int ipd_amg_packed_operator(const ipd_amg* h, int32_t k, int32_t form, double* out, int64_t cap, int32_t* ld,
                            int32_t* seg, int32_t* n, int32_t* nc);
/* Mode 2 only: `cycles` loop bodies in one launch with in-kernel stamps of workgroup 0:
 * stamps[0] shader clocks spent waiting in hand-off sweeps, [1] shader clocks of the launch,
 * [2] hand-offs, [3] 100 MHz ticks of the launch, [4] clocks in the barrier ahead of the
 * publish (the wave's wait for the workgroup's slowest row), [5] in the store phase,
 * [6] in the closing barrier, [7] in the CSR row walks of the two transfers, [8] in the tail
 * level's solve; [9] in the finishing lanes of the column-slice half sweeps (16-entry rows; with a
 * remote tail: the tail workgroup's busy clocks); the rest is the row work.  total_ms: HIP events. */
int ipd_amg_bench_resident(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                           double* total_ms, int64_t stamps[10]);
/* The same launch, and the stamps by class of hand-off that the column-slice kernels (k_resident<16,16,0[,true]>)
 * take with it (zeros from the other kernels): stamps[0 .. 9] as above, stamps[16 + c] workgroup 0's shader clocks
 * from the start of the own work of a hand-off of class c to the start of the next hand-off's, stamps[24 + c] the
 * hand-offs of class c.  Classes: 0 a level-1 half sweep published behind the barrier of the hand-off before it,
 * 1 the first half sweep of a run (its totals come from LDS, behind a barrier of its own), 2 rr = r - A e, 3 the
 * restriction, 4 level 2 (the composed pass, or each sweep, and the residual with the tail behind it), 5 the
 * prolongation, 6 r = b - A x.  The counts add up to stamps[2]; the clocks add up to stamps[1] less the prologue
 * and the additions of the correction.  Stamps cost LDS operations on the chain: timings come from
 * ipd_amg_bench_cycles.                                                                                      */
int ipd_amg_bench_resident_classes(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                                   double* total_ms, int64_t stamps[32]);

/* Wall-clock attribution of the driver's phases when IPD_PROFILE=1 (each phase is then
 * bracketed by stream synchronisations).  Slots: 0 ASAt, 1 build Ae, 2 components,
 * 3 AMG setup, 4 AMG solve, 5 small-block direct solves, 6 evaluation passes,
 * 7 begin/end passes.  Returns the number of slots.                             */
int ipd_prof_read(double* seconds, int64_t* calls, int32_t reset);

/* ---- multi-GPU row-block sharding (RCCL over xGMI) ----------------------- */
#define IPD_COMM_ID_BYTES 128
int ipd_comm_get_unique_id(uint8_t id[IPD_COMM_ID_BYTES]);
int ipd_comm_init(ipd_ctx*, const uint8_t id[IPD_COMM_ID_BYTES], int rank, int nranks);
int ipd_comm_finalize(ipd_ctx*);
/* Rank and size as RCCL reports them for the context's communicator, and the all-gathers issued
 * on it so far: grouped launches and the vectors inside them; reset != 0 zeroes the counts.   */
int ipd_comm_stats(ipd_ctx*, int32_t* rank, int32_t* nranks, int64_t* allgather_calls,
                   int64_t* allgather_vectors, int32_t reset);
/* Row-block sharded variant of ipd_amg_bench_cycles: every rank holds the same
 * hierarchy, owns rows [rank*N_k/G, (rank+1)*N_k/G) of every level, and the
 * iterate is re-assembled with ncclAllGather after each smoother half-sweep.  */
int ipd_amg_bench_cycles_sharded(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                                 double* total_ms, double* bytes_per_cycle);

#ifdef __cplusplus
}
#endif
#endif /* IPD_AMG_H */
