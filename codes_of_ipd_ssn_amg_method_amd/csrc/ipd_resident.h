// Level-resident solve kernel (a template: ipd_resident_k2.hip and ipd_resident_k3.hip instantiate it).
//
// The multi-launch path pays one kernel boundary plus 2-3 dependent memory round trips per
// half sweep: 4.6-5.0 us per k_smooth launch at m=n=1024, rho=1, where the 12.7 MB a launch
// streams would take 1.6 us at HBM peak (profiles/r1_kernel_stats.csv).  The whole hierarchy of
// that regime (levels 2048 / 1024 / 1: 21 MB + 10.5 MB of padded rows) fits in the chip's
// registers, so this kernel keeps it there for the WHOLE Class_AMG solve:
//
//   * G <= 256 workgroups of 512 threads, one per CU, all co-resident; a wave owns one row of
//     each row block (level 1: F rows and C rows of the bigraph Gauss-Seidel, level 2: Jacobi),
//     lane l holds entries l, l+64, ... of the padded row (16-bit column, fp64 value) in VGPRs;
//   * every workgroup keeps the full vectors of both levels (x, e, r, r - A e, A*1) in LDS, so a
//     row dot product is LDS gathers + one DPP wave sum, no memory traffic at all;
//   * 16-entry rows (the dense regime, the metric's workload): level 1 is held turned by 90 degrees, in
//     COLUMN SLICES -- thread t, which polls granules t and t + 512 of a block, holds columns t and t + 512
//     of the (at most 8) rows its workgroup owns in the other block, densely: 32 doubles, what the two row
//     slices cost, and no column registers.  A received value is multiplied in the register it arrived in,
//     a transposing butterfly (res_cs_rows) leaves the waves' row totals in LDS, and after ONE barrier
//     lanes 0..7 of wave 0 add them, finish the rows and publish the next half sweep from registers
//     (half1_cs): no gather phase, no store phase, no closing barrier and no trip of the published values
//     through LDS remain on a half sweep's chain.  The other kernels keep a row per wave;
//   * the only global traffic is the hand-off of each half sweep's result: tagged 16-byte granules that every
//     workgroup publishes and sweeps, two buffers by step parity (ipd_resident_proto.h describes the protocol,
//     its bounded spins and the give-up word);
//   * the kernel-space scalar c = 1'(r - A e)/xx of the next sweep is reduced in the same sweep
//     phase that stores the new iterate (no extra barrier), the transfers to and from level 2 walk
//     the CSR rows of P'/P from L2 (twice per cycle), and the tail level (<= 64 rows, 1 row in
//     the dense regime) is solved redundantly by every workgroup, so it needs no hand-off;
//   * the stationary iteration and its stopping rules (Class_AMG.m:86-109) run in the kernel
//     (res_stationary, ipd_resident_proto.h): one launch and one read-back per solve.
//
// Arithmetic per row is the multi-launch kernels' (phase_smooth / phase_resid / phase_xfer /
// phase_top), only the order inside a row's dot product differs (lane-strided entries).
#pragma once

#include "ipd_resident_proto.h"

static constexpr int RES_P3_LD = 1152;         // row stride of ResDesc::p3rows: 512 + 512 + 128
static constexpr int RES_P4_LD = 2 * RES_P4_SEG + 64;

struct ResLevelDesc {
    int N, nf, S;
    const unsigned short* pci;
    const double* pva;
    const double* diag;
    const double* dinv;
    const double* Axi;
    const double* xx;
};
struct ResDesc {
    ResLevelDesc L1, L2;
    ResLevelDesc L3;  // third resident level (Jacobi, <= BT rows), `three` != 0 only
    ResCsr Pt2, P2;   // level 1 <-> 2: restriction rows (N2 x N1), prolongation rows (N1 x N2)
    ResCsr Pt3, P3;   // level 2 <-> 3 (the tail level of a three-level hierarchy)
    ResCsr Pt4, P4;   // level 3 <-> 4 (`three` only: the remote tail is rooted at level 4)
    ResCsr A3;        // tail operator (CSR), local tail only
    ResCsr A4;        // ... when level 3 is resident too and level 4 is the (local) tail
    int three;        // levels 1-3 resident (hierarchies whose level 3 does not fit the tail's LDS)
    // Level 3 in polynomial form (template argument KE3 == 1, remote tail only; pack_bpoly with rows):
    // row i < N3 of p3rows is [M2a | M1](i,:) and row N3 + c is the restriction row c stacked on it,
    // entries 0..N3-1 applied to r_3, 512..512+N3-1 to e_3 and (rows < N3) 1024..1024+N4-1 = (M1 P4)(i,:)
    // to the tail's e_4 (row stride RES_P3_LD); p3w their factors of 1'r_3.  A visit of level 3 is then
    // THREE hand-offs (e' and the restricted residual; the tail's answer e_4 -- the tail workgroup does not
    // prolongate in this mode --; e'') instead of thirteen (ten sweeps, the residual, the restriction, the
    // prolongation).
    const double* p3rows;
    const double* p3w;
    // Level 2 in polynomial form, COMPOSED over a whole visit (template argument POLY2; three levels with a
    // one-row tail, V cycle -- the metric's workload; ipd_amg_attach_level2_poly).  The nu pre-sweeps, the
    // residual, the restriction to the one-row tail, its prolongation and the nu post-sweeps of a visit that
    // starts from e = 0 (AMG/MG_Vcycle.m:14-41) are the affine map
    //     e_2 = B r_2 + wB (1'r_2) + mp e_3,   e_3 = PCG(h33, s'r_2 + ws (1'r_2)),
    // B = M1 M2a + M2a, wB = M1 w + w, mp = M1 p3, s = P3' - (P3'A) M2a (pack_bpoly's operators, one more dense
    // product): row i of p2rows holds B(i,:) at [p2seg ..), mp_i at [2 p2seg], row N2 holds s; p2w = [wB; ws].
    // A visit of level 2 is then ONE hand-off instead of ten.
    const double* p2rows;
    const double* p2w;
    int p2seg, p2ld;
    // Level 4 in polynomial form in the resident workgroups as well (round 4, POLY3 hierarchies of six levels
    // and more; N5 > 0): row b < N4 of [M2a | M1] and the restriction row N4 + b (b < N5) per workgroup, fetched
    // from L2 at every pass (row stride RES_P4_LD: [Mr (128) | Me (128) | Mc (64)]); the restricted residual of
    // level 3 goes to EVERYBODY in the ack granules of level 3's hand-off, and the tail workgroup is rooted
    // at level 5 (ResTail::sub then holds levels 5..J, root = 5).  With the tail at level 4 its two legs
    // per visit of level 3 were 50 us of serial work on the late Newton systems (4 per W cycle: 200 of 296 us).
    int N5;
    const double* p4rows;
    const double* p4w;
    // Remote tail (hierarchies with more than three levels): workgroup gridDim.x - 1 serves the visits of
    // everything below the resident levels (ipd_resident_proto.h): rooted at level 3, the other workgroups hand
    // it r_3 = P3' rr_2 (Nt granules) and receive the prolongated correction P3 e_3 (N2 granules).
    int remote;
    ResTail tail;     // what that workgroup reads and the wire to it
    // Level 1 <-> 2 transfers from the active-set bit mask (amg_attach_maskop, three-level hierarchies
    // with bigraph transfers only): W(j,i) = s_ij beta_i rho_j (AMG/transfer.m:19-25 on Hybrid_AMG's
    // rescaled operator), so a row of P' or P is 1 bit per entry -- 16 bits per lane, held in one
    // register -- against a pre-scaled LDS vector, instead of a CSR row walked from L2 (12.6 MB per
    // cycle, 5 us of a 72 us cycle).  xm != 0: fbits / cbits as MaskOp (row-major 64-bit words).
    int xm, xm_nwf, xm_nwc;
    const unsigned long long* xm_fbits;
    const unsigned long long* xm_cbits;
    const double* xm_beta;   // nc: the C node's factor
    const double* xm_rho;    // nf: the F row's factor (1 / row sum with isnsp)
    int localfirst;   // zero-start first sweeps formed locally (see k_resident); 0: handed off like the rest
    int wident;       // P = [W; I] verified (k_res_check_ident): identity entries are added, not walked
    int Nt;           // rows of the tail level (local tail) or of the remote tail's root level
    int nu, isnsp, wcycle, anycycle, maxit;
    double retol;
    long long pcg_maxit;
    unsigned char* gran0;
    unsigned char* gran1;
    int presleep;       // s_sleep(1) repetitions between a publish and the first poll of its sweep
    int pollsleep;      // ... and between two polls
    unsigned* tmo;      // [0] != 0: a bounded spin gave up (value = step number)
    long long* dbg;     // optional stamps (diagnostic build of the bench): see k_resident
    unsigned dbg_skip_seq;   // test hook (IPD_RES_DEBUG_SKIP_PUBLISH=<step>): the last workgroup omits its
                             // publish of that step, so every sweep of the step gives up; 0 = off
};

// lane-strided slice of one padded row: entries lane, lane+64, ... ; the 16-bit columns are kept
// as LDS byte offsets (8*column <= 16376), two per register
template <int KE>
__device__ __forceinline__ void res_load_slice(const ResLevelDesc& L, int row, bool valid, int lane,
                                               unsigned (&c)[KE / 2], double (&a)[KE]) {
    unsigned cc[KE];
#pragma unroll
    for (int q = 0; q < KE; ++q) {
        const int e = lane + 64 * q;
        const bool ok = valid && e < L.S;
        const size_t off = ok ? (size_t)row * L.S + e : 0;
        const unsigned short cj = L.pci[off];
        const double aa = L.pva[off];
        cc[q] = ok ? 8u * cj : 0u;
        a[q] = ok ? aa : 0.0;
    }
#pragma unroll
    for (int q = 0; q < KE / 2; ++q) c[q] = cc[2 * q] | (cc[2 * q + 1] << 16);
}

// row dot product against the LDS vector at byte offset OFFB (a compile-time constant below
// 64 KB: one ds_read_b64 with an immediate offset per entry)
template <int KE, int OFFB>
__device__ __forceinline__ double res_rowdot(unsigned (&c)[KE / 2], const double (&a)[KE],
                                             const char* smb) {
    double y[KE];
#pragma unroll
    for (int q = 0; q < KE / 2; ++q) {
        // opaque: keeps the unpacked offsets from being hoisted out of the cycle loops (they
        // would cost a register per matrix entry for the whole kernel)
        asm volatile("" : "+v"(c[q]));
        const unsigned lo = c[q] & 0xffffu, hi = c[q] >> 16;
        y[2 * q] = *reinterpret_cast<const double*>(smb + OFFB + lo);
        y[2 * q + 1] = *reinterpret_cast<const double*>(smb + OFFB + hi);
    }
    // four partial sums (entries q, q+4, ...): the dependent add chain is a quarter as long
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int q = 0; q < KE; q += 4) {
        s0 += a[q] * y[q];
        s1 += a[q + 1] * y[q + 1];
        s2 += a[q + 2] * y[q + 2];
        s3 += a[q + 3] * y[q + 3];
    }
    return (s0 + s1) + (s2 + s3);
}

// The same dot product with fused multiply-adds, each partial sum seeded with its first product
// (k_resident's half sweeps): 4 v_mul_f64 + 12 v_fmac_f64 per lane instead of 16 multiplies and 16 adds,
// four of them adds to 0.0 -- half the fp64 instructions the two waves of a SIMD issue per row dot, and a
// dependent chain per partial sum half as long.
template <int KE, int OFFB>
__device__ __forceinline__ double res_rowdot_fma(unsigned (&c)[KE / 2], const double (&a)[KE],
                                                 const char* smb) {
    static_assert(KE % 4 == 0, "four partial sums");
    double y[KE];
#pragma unroll
    for (int q = 0; q < KE / 2; ++q) {
        asm volatile("" : "+v"(c[q]));   // (see res_rowdot)
        const unsigned lo = c[q] & 0xffffu, hi = c[q] >> 16;
        y[2 * q] = *reinterpret_cast<const double*>(smb + OFFB + lo);
        y[2 * q + 1] = *reinterpret_cast<const double*>(smb + OFFB + hi);
    }
    double s0 = a[0] * y[0], s1 = a[1] * y[1], s2 = a[2] * y[2], s3 = a[3] * y[3];
#pragma unroll
    for (int q = 4; q < KE; q += 4) {
        s0 = __builtin_fma(a[q], y[q], s0);
        s1 = __builtin_fma(a[q + 1], y[q + 1], s1);
        s2 = __builtin_fma(a[q + 2], y[q + 2], s2);
        s3 = __builtin_fma(a[q + 3], y[q + 3], s3);
    }
    return (s0 + s1) + (s2 + s3);
}

// CSR row of a transfer operator (global, L2-resident) against an LDS vector, one wave per row
__device__ __forceinline__ double res_csr_rowdot(const ResCsr& M, int e0, int e1, int lane,
                                                 const double* sm, int off) {
    double s = 0.0;
    for (int t = e0 + lane; t < e1; t += 64 * 8) {   // 8 entries per lane in flight: a 1025-entry row = 3 trips
        int jj[8];
        double aa[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int tt = t + 64 * u;
            const int tc = tt < e1 ? tt : e0;
            jj[u] = M.ci[tc];
            aa[u] = M.va[tc];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (t + 64 * u < e1) ? aa[u] * sm[off + jj[u]] : 0.0;
    }
    return wave_sum(s);
}

// Block sums of up to two per-thread partials through red[0..2*RES_WAVES): the caller has
// written red[w] / red[RES_WAVES + w] before the barrier that precedes this call.
__device__ __forceinline__ double res_red8(const double* red) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < RES_WAVES; ++k) t += red[k];
    return t;
}

// The same sum as a fixed pairwise tree (k_resident's hand-offs): the eight reads are issued together and
// three dependent adds follow, where the sequential form became four LDS round trips and eight dependent
// adds, the first of them to 0.0, between the closing barrier and the next row dot.  Every workgroup adds
// in the same order, so every workgroup gets the same bits.
__device__ __forceinline__ double res_red8_tree(const double* red) {
    static_assert(RES_WAVES == 8, "eight waves");
    double v[RES_WAVES];
#pragma unroll
    for (int k = 0; k < RES_WAVES; ++k) v[k] = red[k];
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// ---- column slices (k_resident with 16-entry rows: level 1 turned by 90 degrees) ----------------------
// Thread t holds columns t and t + BT of the (at most RES_WAVES) rows its workgroup owns in a block, so a
// value that thread t has just received -- or read from LDS -- meets its matrix entries in the register it
// arrived in.  res_cs_rows forms the workgroup's row totals from two such values per thread:
//   1. part[r] = A[r][0] v0 + A[r][1] v1: one multiply and one fused multiply-add per row;
//   2. a transposing butterfly over the wave: 8 -> 4 values (permlane32 swap: the lower half of the wave keeps
//      rows 0..3, the upper half rows 4..7), 4 -> 2 (permlane16 swap), 2 -> 1 (DPP row_ror:8), then three more
//      DPP steps on the single value: lanes 8 r .. 8 r + 7 end up with the wave's total of row r;
//   3. lane 8 r writes it to part_out[8 r + w].
// After the caller's barrier res_red8_tree(part_out + 8 r) is row r's sum over all columns.  Map, butterfly and
// tree are the same in every workgroup, so every workgroup forms the same bits from the same values.
__device__ __forceinline__ void res_swap_halves32(double& a, double& b) {
    // lanes 32..63 of a <-> lanes 0..31 of b
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void res_swap_rows16(double& a, double& b) {
    // odd 16-lane rows of a <-> even 16-lane rows of b
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    a = __hiloint2double((int)hi[0], (int)lo[0]);
    b = __hiloint2double((int)hi[1], (int)lo[1]);
}
__device__ __forceinline__ void res_cs_rows(const double (&A)[RES_WAVES][2], double v0, double v1, double* part_out,
                                            int w, int lane) {
    static_assert(RES_WAVES == 8, "eight rows per block and workgroup");
    double p[RES_WAVES];
#pragma unroll
    for (int r = 0; r < RES_WAVES; ++r) p[r] = __builtin_fma(A[r][1], v1, A[r][0] * v0);
    double q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // lanes 0..31: rows k, lanes 32..63: rows k + 4
        res_swap_halves32(p[k], p[k + 4]);
        q[k] = p[k] + p[k + 4];
    }
    double t[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {   // 16-lane rows 0..3 of the wave: rows k, k + 2, k + 4, k + 6
        res_swap_rows16(q[k], q[k + 2]);
        t[k] = q[k] + q[k + 2];
    }
    const bool f = (lane & 8) != 0;   // lanes 8..15 of a 16-lane row keep the odd row
    const double keep = f ? t[1] : t[0], send = f ? t[0] : t[1];
    double u = keep + dpp_get<0x128, 0xf>(send);   // row_ror:8 -- the value of lane ^ 8
    u = subwave_sum(u, 8);
    if ((lane & 7) == 0) part_out[8 * (lane >> 3) + w] = u;
}

// Classes of chip-wide hand-offs, for the stamps by class (ipd_amg_bench_resident_classes, column-slice kernels):
// workgroup 0 charges the clocks from the start of a hand-off's own work to the start of the next one's to its class.
enum res_class {
    RES_CL_HALF = 0,    // a level-1 half sweep published behind the barrier of the hand-off before it
    RES_CL_START = 1,   // ... the first of a run: its totals come from LDS behind a barrier of its own
    RES_CL_RR = 2,      // rr = r - A e
    RES_CL_RESTRICT = 3,   // r_2 = P' rr
    RES_CL_LEVEL2 = 4,  // level 2: the composed pass, or each of its sweeps and its residual (with the tail)
    RES_CL_PROLONG = 5, // e_1 += P e_2
    RES_CL_TOP = 6,     // r = b - A x
    RES_NCLASS = 8
};

// out[0] = it, out[1] = rel_res, out[2] = res0; rel_resk at out[4 ..], rhok at out[4+maxit+2 ..]
// (res_stationary; the last slot: hand-offs of the launch).  fixed_cycles > 0: the bench hook.  dbg (optional, 16 words): [0] shader clocks spent waiting in sweeps by
// workgroup 0, [1] clocks of the whole loop, [2] number of hand-offs, [3] 100 MHz ticks of the loop,
// [4] clocks in the barrier before the publish, [5] in the store phase, [6] in the closing barrier, [9] in the
// finishing lanes of the column-slice half sweeps (whose one barrier counts as [4], their receipt as [5]).
// Column slices: dbg has 32 words, [16 + c] the clocks and [24 + c] the hand-offs of class c (res_class).
//
// DIAG: the stamps and the skip-publish test hook are in the code (a launch asks for them through D.dbg /
// D.dbg_skip_seq); false: the production form of the column-slice kernels, none of it compiled in.
// FULL (POLY2 only, resident_takes_full): the metric's full shape -- nf = nc = N2 = 2 BT, G RES_WAVES = nf, mask-form
// transfers with P = [W; I], isnsp, local first sweeps, nu >= 1, one-row local tail.  Sizes, row ranges and mode flags
// are then constants: no bound, no clamp, no mode select and no CSR alternative is left in the cycle loop, and the
// tail workgroup's code is not in the kernel.  Arithmetic and the order of every sum are the general form's.  The hand-offs
// between the runs of half sweeps are fed there as well: rr rides the pre run's last half sweep and top (with x += e) the post
// run's (half1_cs), the prolongation sends its F block only, and the pre run starts from top's local first half.
template <int KE1, int KE2, int KE3 = 0, bool POLY2 = false, bool DIAG = true, bool FULL = false>
__global__ __launch_bounds__(BT, 2) void k_resident(const ResDesc D, const double* __restrict__ bvec,
                                                    double* xg, double* out, int fixed_cycles) {
    static_assert(!POLY2 || (KE3 == 0 && KE1 == 16), "POLY2: three-level hierarchies in column slices (resident_takes_poly2)");
    static_assert(!FULL || POLY2, "FULL: the composed instantiation only (resident_takes_full)");
    static_assert(DIAG || KE1 == 16, "the production form exists for the column-slice kernels");
    constexpr int FG = 2 * BT / RES_WAVES;   // FULL: workgroups, each with RES_WAVES rows of every block
    if constexpr (FULL) __builtin_assume(__builtin_amdgcn_workitem_id_x() < (unsigned)BT);
    constexpr bool THREE = KE3 > 0;
    constexpr bool POLY3 = KE3 == 1;   // level 3 in polynomial form (ResDesc::p3rows)
    constexpr int K3 = (THREE && !POLY3) ? KE3 : 2;
    extern __shared__ __attribute__((aligned(16))) char res_smem[];
    double* sm = reinterpret_cast<double*>(res_smem);
    const char* smb = res_smem;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    // (macros, not variables or lambdas: in the general forms they leave the very expressions that stood here, so
    // the encodings of those kernels do not change)
#define RES_REMOTE (FULL ? 0 : D.remote)
#define RES_WIDENT (FULL ? 1 : D.wident)
    const int b = blockIdx.x, G = FULL ? FG : gridDim.x - (RES_REMOTE ? 1 : 0);   // G: workgroups of levels 1-2
    const int N1 = FULL ? 4 * BT : D.L1.N, N2 = FULL ? 2 * BT : D.L2.N, nf = FULL ? 2 * BT : D.L1.nf, nc = N1 - nf;
    const int Nt = FULL ? 1 : D.Nt;
    if (RES_REMOTE && b == G) {   // the tail workgroup
        __shared__ PhaseLds tail_lds;
        __shared__ double tail_red[16];
        __shared__ double tail_part[48 + SOLVE_ML + 1];
        __shared__ int tail_stat[RES_WAVES];
        res_tail_workgroup(D.tail, res_smem, &tail_lds, tail_red, tail_part, tail_stat);
        return;
    }
    // LDS map (doubles): fixed slots of RES_NMAX entries, the gather targets in the first 64 KB so
    // that a gather is one ds_read_b64 with an immediate offset (no address arithmetic to hoist)
    constexpr int oX = 0, oE1 = RES_NMAX, oE2 = 2 * RES_NMAX, oRR1 = 3 * RES_NMAX;
    constexpr int oR1 = 4 * RES_NMAX, oAX1 = 5 * RES_NMAX, oR2 = 6 * RES_NMAX, oRR2 = 7 * RES_NMAX;
    constexpr int oAX2 = 8 * RES_NMAX;
    constexpr int oRHO = 9 * RES_NMAX;                 // mask-form transfers: rho of the F rows (nf <= RES_NMAX / 2)
    constexpr int oBETA = oAX2 + RES_NMAX / 2;         // ... beta of the C nodes: upper half of the AX2 slot (!THREE)
    constexpr int oU = oRR2;                           // ... beta .* e_2: lower half of the RR2 slot (free after the visit)
    constexpr int oR3 = 9 * RES_NMAX + RES_NMAX / 2, oE3 = oR3 + RES_TAIL_MAX, oP3 = oE3 + RES_TAIL_MAX;
    // column slices: the waves' row totals, two buffers of RES_WAVES rows x RES_WAVES waves, and the waves' parts of
    // the kernel-space scalar (two buffers by hand-off parity).  They share the tail level's slots: the tail runs
    // between level 2's hand-offs, where no level-1 total is in flight.
    constexpr int oPART = oR3, oPART9 = oR3 + 2 * RES_WAVES * RES_WAVES;
    static_assert(2 * RES_WAVES * RES_WAVES + 2 * RES_WAVES <= 3 * RES_TAIL_MAX, "the totals fit the tail's slots");
    constexpr int oRED = oP3 + RES_TAIL_MAX;          // 2*RES_WAVES doubles
    constexpr int oPUB = oRED + 2 * RES_WAVES;        // values the waves publish this step (2 blocks)
    constexpr int oOWN = oPUB + 2 * RES_WAVES;        // 10 scalars of each wave's rows
    int* fail = reinterpret_cast<int*>(sm + oOWN + 10 * RES_WAVES);
    long long* dbg_acc = reinterpret_cast<long long*>(sm + oOWN + 10 * RES_WAVES + 1);   // 9 words (+1 .. +9; rowp starts at +12)
    // entry ranges of this wave's rows of the transfer operators: read once, a walk then starts
    // with its entries instead of a dependent trip for the row pointers
    int* rowp = reinterpret_cast<int*>(sm + oOWN + 10 * RES_WAVES + 12);                 // 12 ints per wave
    // stamps by class, 32-bit words (a class's clocks of one launch stay far below 2^32, and sums of differences of
    // low words are exact modulo 2^32): clocks [0 .. 8), hand-offs [8 .. 16)
    unsigned* cls_acc = reinterpret_cast<unsigned*>(sm + oOWN + 10 * RES_WAVES + 12 + 6 * RES_WAVES);
    // FULL: a third buffer of row totals behind everything else.  The last half sweep of a run forms the totals of
    // BOTH blocks (they feed rr, or top's r = b - A x): the other block's between its publish and its wait, where the
    // finishing lanes may still be reading the totals of that very publish from buffer csBuf -- so they go here --,
    // and the received block's at its receipt, into buffer csBuf ^ 1 as in every fed half sweep.
    constexpr int oPART3 = oOWN + 10 * RES_WAVES + 12 + 6 * RES_WAVES + 8;
    static_assert(!FULL || sizeof(double) * (oPART3 + RES_WAVES * RES_WAVES) <= RES_LDS_BYTES, "the third buffer lies inside the launch's LDS");
    // third resident level (THREE): its vectors sit in the upper halves of level 2's slots (N2 <= 1024,
    // N3 <= 512); E3 is a gather target and must lie below 64 KB
    constexpr int oE3L = oE2 + RES_NMAX / 2, oR3L = oRR2 + RES_NMAX / 2, oRR3L = oRR2 + 3 * RES_NMAX / 4;
    // POLY4 (the RR3L region holds 512 doubles, e_4 takes 128): r_4, e_5, partial sums and the rows' factors
    constexpr int oR4L = oRR3L + 128, oE5L = oRR3L + 256, oPS4 = oRR3L + 320;
    constexpr int oAX3L = oAX2 + RES_NMAX / 2;
    const int N3 = THREE ? D.L3.N : 0;
    double* red = sm + oRED;

    // ---- rows of this wave ------------------------------------------------------------------
    const int loF = FULL ? b * RES_WAVES : (int)(((long long)b * nf) / G);
    const int hiF = FULL ? loF + RES_WAVES : (int)(((long long)(b + 1) * nf) / G);
    const int loC = FULL ? nf + b * RES_WAVES : nf + (int)(((long long)b * nc) / G);
    const int hiC = FULL ? loC + RES_WAVES : nf + (int)(((long long)(b + 1) * nc) / G);
    const int lo2 = FULL ? b * RES_WAVES : (int)(((long long)b * N2) / G);
    const int hi2 = FULL ? lo2 + RES_WAVES : (int)(((long long)(b + 1) * N2) / G);
    // row l of a block's own rows (every workgroup owns a row of every block: a lane beyond them takes the last)
#define RES_OWN_ROW(lo, hi, l) (FULL ? (lo) + ((l) & (RES_WAVES - 1)) : ((lo) + (l) < (hi) ? (lo) + (l) : (hi) - 1))
    const int rowF = loF + w, rowC = loC + w, row2 = lo2 + w;
    const bool vF = rowF < hiF, vC = rowC < hiC, v2 = row2 < hi2;
    const int rF = vF ? rowF : 0, rC = vC ? rowC : 0, r2 = v2 ? row2 : 0;
    const int lo3 = THREE ? (int)(((long long)b * N3) / G) : 0, hi3 = THREE ? (int)(((long long)(b + 1) * N3) / G) : 0;
    const int row3 = lo3 + w;
    const bool v3 = THREE && row3 < hi3;
    const int r3 = v3 ? row3 : 0;

    // ---- matrix slices -> registers (the only read of the matrices in the whole solve) --------
    // 16-entry rows: level 1 in column slices (see res_cs_rows) -- thread t holds columns nf + t, nf + t + BT of
    // the workgroup's F rows (AF) and columns t, t + BT of its C rows (AC), 32 doubles, and no column registers.
    // The layout has no slot for an entry of an F row in an F column or of a C row in a C column (the bigraph
    // level 1 has none: transfer.m:20-21 needs a diagonal Aff, and the Newton systems' Acc is diagonal too); a
    // hierarchy that has one is reported to the host (out[3] = 2), which drops its resident plan: it runs as launches.
    constexpr bool CS1 = KE1 == 16;
    constexpr int KR1 = CS1 ? 4 : KE1;   // the row-per-wave slices of level 1 (unused with column slices)
    unsigned cF[KR1 / 2], cC[KR1 / 2], c2[KE2 / 2];
    double aF[KR1], aC[KR1], a2[KE2];
    double AF[RES_WAVES][2], AC[RES_WAVES][2];
    (void)cF; (void)cC; (void)aF; (void)aC; (void)AF; (void)AC;
    if constexpr (CS1) {
        // dense slices from the padded rows through LDS (the vector slots are still unused: a block's stage is
        // RES_WAVES rows of 2 BT doubles): zero the stage, wave w scatters row w, every thread reads its columns
        constexpr int SW = 2 * BT;
        bool lost = false;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            for (int i = tid; i < RES_WAVES * SW; i += BT) sm[i] = 0.0;
            __syncthreads();
            const int row = blk == 0 ? rF : rC, c0 = blk == 0 ? nf : 0, ncol = blk == 0 ? nc : nf;
            if (blk == 0 ? vF : vC)
                for (int e = lane; e < D.L1.S; e += 64) {
                    const size_t off = (size_t)row * D.L1.S + e;
                    const int k = (int)D.L1.pci[off] - c0;
                    const double aa = D.L1.pva[off];
                    if (aa != 0.0) {   // (padding entries have value 0)
                        if (k >= 0 && k < ncol && k < SW)
                            sm[w * SW + k] = aa;
                        else
                            lost = true;
                    }
                }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RES_WAVES; ++r)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const double aa = sm[r * SW + tid + u * BT];
                    if (blk == 0) AF[r][u] = aa; else AC[r][u] = aa;
                }
            __syncthreads();
        }
        if (lost) {   // word 1: "the layout cannot hold this matrix" (not a time-out); word 0 ends everybody's waits
            __hip_atomic_store(D.tmo + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(D.tmo, 0x7ffffffeu, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        res_load_slice<KR1>(D.L1, rF, vF, lane, cF, aF);
        res_load_slice<KR1>(D.L1, rC, vC, lane, cC, aC);
    }
    // The composed level 2 is held in column slices as well: thread t holds columns t and t + BT of the workgroup's
    // rows of B -- the 16 doubles the row slice a2 costs the sweep form -- and the received r_2 meets them in the
    // registers it arrived in (poly2_fed).
    double B2[RES_WAVES][2];
    (void)B2;
    if constexpr (POLY2) {
#pragma unroll
        for (int r = 0; r < RES_WAVES; ++r)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int col = tid + u * BT;
                const bool ok = lo2 + r < hi2 && col < N2;
                const double bv = D.p2rows[(size_t)(ok ? lo2 + r : 0) * D.p2ld + D.p2seg + (ok ? col : 0)];
                B2[r][u] = ok ? bv : 0.0;
            }
    } else {
        res_load_slice<KE2>(D.L2, r2, v2, lane, c2, a2);
    }
    unsigned c3[K3 / 2];
    double a3[K3];
    if (THREE && !POLY3) res_load_slice<K3>(D.L3, r3, v3, lane, c3, a3);
    // polynomial form: entries tid and 512 + tid of the workgroup's rows lo3..hi3-1 (at most four) and of
    // restriction row b (the remote tail's root level has at most G rows: one per workgroup)
    double m3r[5], m3e[5], m3c[4];
#pragma unroll
    for (int q = 0; q < 5; ++q) m3r[q] = m3e[q] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) m3c[q] = 0.0;
    if (POLY3) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int row = q < 4 ? lo3 + q : N3 + b;
            const bool ok = (q < 4 ? row < hi3 : b < Nt) && tid < N3;
            if (ok) {
                m3r[q] = D.p3rows[(size_t)row * RES_P3_LD + tid];
                m3e[q] = D.p3rows[(size_t)row * RES_P3_LD + 512 + tid];
            }
            if (q < 4 && row < hi3 && tid < Nt) m3c[q] = D.p3rows[(size_t)row * RES_P3_LD + 1024 + tid];
        }
        if (tid < 5) {
            const int row = tid < 4 ? lo3 + tid : N3 + b;
            sm[oE3 + tid] = (tid < 4 ? row < hi3 : b < Nt) ? D.p3w[row] : 0.0;
        }
        if (D.N5 > 0 && tid < 2) {   // POLY4: the factors of 1'r_4 of row b and of restriction row N4 + b
            const int row = tid == 0 ? b : Nt + b;
            sm[oPS4 + 20 + tid] = (tid == 0 ? b < Nt : b < D.N5) ? D.p4w[row] : 0.0;
        }
    }
    // the rows' own scalars live in LDS (a register pair each would stay live for the whole solve)
    if (lane == 0) {
        sm[oOWN + 0 * RES_WAVES + w] = D.L1.diag[rF];
        sm[oOWN + 1 * RES_WAVES + w] = D.L1.dinv[rF];
        sm[oOWN + 2 * RES_WAVES + w] = bvec[rF];
        sm[oOWN + 3 * RES_WAVES + w] = D.L1.diag[rC];
        sm[oOWN + 4 * RES_WAVES + w] = D.L1.dinv[rC];
        sm[oOWN + 5 * RES_WAVES + w] = bvec[rC];
        sm[oOWN + 6 * RES_WAVES + w] = POLY2 ? D.p2w[r2] : D.L2.diag[r2];                                    // (POLY2: wB)
        sm[oOWN + 7 * RES_WAVES + w] = POLY2 ? D.p2rows[(size_t)r2 * D.p2ld + 2 * D.p2seg] : D.L2.dinv[r2];   // (POLY2: mp)
        sm[oOWN + 8 * RES_WAVES + w] = (THREE && !POLY3) ? D.L3.diag[r3] : 0.0;
        sm[oOWN + 9 * RES_WAVES + w] = (THREE && !POLY3) ? D.L3.dinv[r3] : 0.0;
        rowp[12 * w + 0] = D.Pt2.rp[r2];
        rowp[12 * w + 1] = v2 ? D.Pt2.rp[r2 + 1] - D.wident : D.Pt2.rp[r2];
        rowp[12 * w + 2] = D.P2.rp[rF];
        rowp[12 * w + 3] = vF ? D.P2.rp[rF + 1] : D.P2.rp[rF];
        rowp[12 * w + 4] = D.P2.rp[rC];
        rowp[12 * w + 5] = vC ? D.P2.rp[rC + 1] : D.P2.rp[rC];
        // remote tail: row b + G*w of the restriction to its root level, if there is one
        const int rin = b + G * w;
        const ResCsr& Pin = D.tail.root == 4 ? D.Pt4 : D.Pt3;
        rowp[12 * w + 6] = (RES_REMOTE && rin < Nt) ? Pin.rp[rin] : 0;
        rowp[12 * w + 7] = (RES_REMOTE && rin < Nt) ? Pin.rp[rin + 1] : 0;
        // third resident level: its own row of P3' (restriction 2 -> 3), this wave's level-2 row of P3
        rowp[12 * w + 8] = v3 ? D.Pt3.rp[r3] : 0;
        rowp[12 * w + 9] = v3 ? D.Pt3.rp[r3 + 1] : 0;
        rowp[12 * w + 10] = (THREE && v2) ? D.P3.rp[r2] : 0;
        rowp[12 * w + 11] = (THREE && v2) ? D.P3.rp[r2 + 1] : 0;
    }
#define dgF sm[oOWN + 0 * RES_WAVES + w]
#define dvF sm[oOWN + 1 * RES_WAVES + w]
#define bF sm[oOWN + 2 * RES_WAVES + w]
#define dgC sm[oOWN + 3 * RES_WAVES + w]
#define dvC sm[oOWN + 4 * RES_WAVES + w]
#define bC sm[oOWN + 5 * RES_WAVES + w]
#define dg2 sm[oOWN + 6 * RES_WAVES + w]
#define dv2 sm[oOWN + 7 * RES_WAVES + w]
#define dg3 sm[oOWN + 8 * RES_WAVES + w]
#define dv3 sm[oOWN + 9 * RES_WAVES + w]
    const bool nsp = FULL ? true : D.isnsp != 0;
    const double xx1 = nsp ? D.L1.xx[0] : 1.0, xx2 = nsp ? D.L2.xx[0] : 1.0;
    const double xx3 = (THREE && nsp) ? D.L3.xx[0] : 1.0;
    // the kernel-space scalars of the hand-offs are formed as sum * (1 / xx): a multiply where a division
    // (thirteen dependent instructions) stood between the closing barrier and the next row dot
    const double rxx1 = 1.0 / xx1, rxx2 = 1.0 / xx2, rxx3 = 1.0 / xx3;
    for (int j = tid; j < N1; j += BT) {
        sm[oX + j] = xg[j];
        sm[oE1 + j] = 0.0;
        sm[oAX1 + j] = D.L1.Axi[j];
    }
    for (int j = tid; j < N2; j += BT) {
        sm[oE2 + j] = 0.0;
        sm[oAX2 + j] = D.L2.Axi[j];
    }
    if (THREE)
        for (int j = tid; j < N3; j += BT) {
            sm[oE3L + j] = 0.0;
            sm[oAX3L + j] = D.L3.Axi[j];
        }
    // One-row tail (the dense regimes): its transfer operator is one column, kept densely in the
    // unused upper half of the RR2 slot (restriction and prolongation use the same numbers), and
    // its operator is one number: the tail then costs two LDS passes instead of five dependent
    // trips to L2 per visit.
    const bool tail1 = FULL ? true : !THREE && Nt == 1 && N2 <= RES_NMAX / 2;
    constexpr int oP3C = oRR2 + RES_NMAX / 2;
    // First sweep of a visit (zero start): e = D^-1 (r - (A 1) c) needs no matrix row, so every
    // workgroup forms ALL its entries itself from the r it has just received -- no hand-off.  The
    // inverse diagonals of the F rows of level 1 and of level 2 sit in the unused upper halves of
    // the R2 / E2 slots (same condition as tail1's column: at most RES_NMAX / 2 rows).
    const bool lfirst = FULL ? true : D.localfirst && D.nu >= 1 && N2 <= RES_NMAX / 2 && nf <= RES_NMAX / 2;
    const bool lfirst2 = lfirst && !THREE;   // (DV2 shares the upper half of the E2 slot with E3)
    constexpr int oDV1 = oR2 + RES_NMAX / 2, oDV2 = oE2 + RES_NMAX / 2;
    if (lfirst) {
        for (int j = tid; j < nf; j += BT) sm[oDV1 + j] = D.L1.dinv[j];
        if (lfirst2)
            for (int j = tid; j < N2; j += BT) sm[oDV2 + j] = D.L2.dinv[j];
    }
    // mask-form transfers: this wave's F-row bits over the C nodes (low half) and its C-row bits over the
    // F rows (high half); bit q of a half <-> entry lane + 64 q, the layout of the register slices
    const bool xm = FULL ? true : !THREE && D.xm != 0 && nc == N2 && D.wident != 0;
    unsigned xbits = 0;
    if (xm) {
        // (all 32 words requested in one burst: a loop of dependent loads cost ~1 us per word)
        unsigned long long wf[16], wc[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            wf[q] = D.xm_fbits[(size_t)rF * D.xm_nwf + (q < D.xm_nwf ? q : 0)];
            wc[q] = D.xm_cbits[(size_t)(rC - nf) * D.xm_nwc + (q < D.xm_nwc ? q : 0)];
        }
        unsigned lo = 0, hi = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            lo |= (vF && q < D.xm_nwf) ? (unsigned)((wf[q] >> lane) & 1ull) << q : 0u;
            hi |= (vC && q < D.xm_nwc) ? (unsigned)((wc[q] >> lane) & 1ull) << q : 0u;
        }
        xbits = lo | (hi << 16);
        for (int j = tid; j < nf; j += BT) sm[oRHO + j] = D.xm_rho[j];
        for (int j = tid; j < nc; j += BT) sm[oBETA + j] = D.xm_beta[j];
    }
    double h33 = 0.0;
    if (tail1) {
        for (int j = tid; j < N2; j += BT) {
            double v = 0.0;
            if (POLY2) {
                v = D.p2rows[(size_t)N2 * D.p2ld + j];   // the stacked restriction row s
            } else {
                for (int t = D.P3.rp[j]; t < D.P3.rp[j + 1]; ++t)
                    if (D.P3.ci[t] == 0) v = D.P3.va[t];
            }
            sm[oP3C + j] = v;
        }
        for (int t = D.A3.rp[0]; t < D.A3.rp[1]; ++t)
            if (D.A3.ci[t] == 0) h33 = D.A3.va[t];
    }
    if (tid == 0) *fail = 0;
    __syncthreads();

    const auto rs = __builtin_amdgcn_make_buffer_rsrc(D.gran0, 0, 2 * RES_GRAN_MAX * 16, 0x00020000);
    unsigned seq = 0;       // number of the last hand-off
    bool dead = false;      // a spin gave up somewhere: skip every further wait
    const bool dbg = DIAG && D.dbg != nullptr && b == 0 && tid == 0;
    // the test hook (ResDesc::dbg_skip_seq): the last workgroup omits its publish of hand-off sq
#define RES_SKIPPED(sq) (DIAG && (sq) == D.dbg_skip_seq && b == G - 1)
    if (dbg) {
        dbg_acc[0] = dbg_acc[3] = dbg_acc[4] = dbg_acc[5] = dbg_acc[6] = dbg_acc[7] = dbg_acc[8] = 0;
        dbg_acc[1] = __builtin_amdgcn_s_memtime();
        dbg_acc[2] = __builtin_amdgcn_s_memrealtime();
        if constexpr (KE1 == 16)
            for (int k = 0; k < 2 * RES_NCLASS; ++k) cls_acc[k] = 0u;
    }
    // start and end of a hand-off of class c (the end of one is the start of the next): LDS adds without a result,
    // so a stamp holds two registers and no state
    auto cls_begin = [&](int c) __attribute__((always_inline)) {
        if constexpr (KE1 == 16) {
            if (dbg) __hip_atomic_fetch_sub(cls_acc + c, (unsigned)__builtin_amdgcn_s_memtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    };
    auto cls_end = [&](int c) __attribute__((always_inline)) {
        if constexpr (KE1 == 16) {
            if (dbg) {
                __hip_atomic_fetch_add(cls_acc + c, (unsigned)__builtin_amdgcn_s_memtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(cls_acc + RES_NCLASS + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    };

    // ---- hand-off wrapper: sweep + barrier + store + (optional) block sums + barrier ------------
    // STORE(j, v) is called for every granule of the thread; EXTRA() runs once per thread (fix-ups on
    // rows the thread does not sweep); both may add to p0 / p1, whose block totals are returned in
    // t0 / t1.  Nothing reads the vectors between the publish barrier and the closing barrier, so
    // whatever does not need the received values runs BEFORE the wait, where it hides under the
    // hand-off latency: EXTRA, and PRE(j), which RES_HANDOFF_P calls for every granule to read the
    // LDS operands of STORE into pa_[u_] / pb_[u_].  The store phase after the wait is then register
    // arithmetic and LDS writes only (a read there was a dependent LDS round trip per granule on the
    // critical path).
    // The waves have left their values in sm[oPUB + w] (first block) / sm[oPUB + RES_WAVES + w]
    // (second block); after the barrier -- which also ends the step's reads of the vectors that
    // are about to change -- wave 0 publishes them: one store instruction, one 128-byte segment per
    // block (a store per wave would be eight 16-byte partial-line writes: measured 2.6 us of waiting
    // per hand-off against 1.4).  gA/cA, gB/cB: first granule and row count of the two blocks.
#define RES_HANDOFF(NJ, n, gA, cA, gB, cB, STORE, EXTRA, want_sums, t0, t1)                        \
    RES_HANDOFF_P(NJ, n, gA, cA, gB, cB, {}, STORE, EXTRA, want_sums, t0, t1)
#define RES_HANDOFF_P(NJ, n, gA, cA, gB, cB, PRE, STORE, EXTRA, want_sums, t0, t1)                 \
    RES_HANDOFF_PV(NJ, n, gA, cA, gB, cB, sm[oPUB + lane], PRE, STORE, EXTRA, want_sums, t0, t1)
    // PUBV: the value lane 8 * block + row of wave 0 publishes (column slices: formed in the lane from PART)
#define RES_HANDOFF_PV(NJ, n, gA, cA, gB, cB, PUBV, PRE, STORE, EXTRA, want_sums, t0, t1)          \
    RES_HANDOFF_PVA(NJ, n, gA, cA, gB, cB, PUBV, PRE, STORE, {}, EXTRA, want_sums, t0, t1)
    // AFTER: runs once per thread behind the STOREs, ahead of the closing barrier (what the received values feed)
#define RES_HANDOFF_PVA(NJ, n, gA, cA, gB, cB, PUBV, PRE, STORE, AFTER, EXTRA, want_sums, t0, t1)  \
    do {                                                                                           \
        double hv_[NJ], pa_[NJ], pb_[NJ];                                                          \
        (void)pa_;                                                                                 \
        (void)pb_;                                                                                 \
        ++seq;                                                                                     \
        /* a give-up of the previous hand-off (its closing barrier has ordered the flag): read here, where the */ \
        /* LDS round trip hides under the barrier, not behind the closing barrier on the critical path          */ \
        if (*fail) dead = true;                                                                    \
        if (dbg) dbg_acc[3] -= __builtin_amdgcn_s_memtime();                                       \
        __syncthreads();                                                                           \
        if (dbg) dbg_acc[3] += __builtin_amdgcn_s_memtime();                                       \
        if (w == 0) {                                                                              \
            const int l8_ = lane & (RES_WAVES - 1);                                                \
            const bool second_ = lane >= RES_WAVES;                                                \
            if (lane < 2 * RES_WAVES && l8_ < (second_ ? (cB) : (cA)) &&                           \
                !RES_SKIPPED(seq))                                                                 \
                res_publish(rs, seq, (second_ ? (gB) : (gA)) + l8_, (PUBV));                       \
        }                                                                                          \
        double p0 = 0.0, p1 = 0.0;                                                                 \
        _Pragma("unroll") for (int u_ = 0; u_ < NJ; ++u_) {                                        \
            const int j = tid + u_ * BT;                                                           \
            if (j < (n)) { PRE; }                                                                  \
        }                                                                                          \
        EXTRA;                                                                                     \
        if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();                                       \
        for (int ps_ = 0; ps_ < D.presleep; ++ps_) __builtin_amdgcn_s_sleep(1);                    \
        if (res_sweep<NJ>(rs, seq, (n), dead, D.tmo, hv_, D.pollsleep)) {                             \
            *fail = 1;                                                                             \
            if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
        }                                                                                          \
        if (dbg) {                                                                                 \
            const long long t_ = __builtin_amdgcn_s_memtime();                                     \
            dbg_acc[0] += t_;                                                                      \
            dbg_acc[4] -= t_;                                                                      \
        }                                                                                          \
        _Pragma("unroll") for (int u_ = 0; u_ < NJ; ++u_) {                                        \
            const int j = tid + u_ * BT;                                                           \
            if (j < (n)) {                                                                         \
                const double v = hv_[u_];                                                          \
                STORE;                                                                             \
            }                                                                                      \
        }                                                                                          \
        AFTER;                                                                                     \
        if (want_sums) {                                                                           \
            p0 = wave_sum(p0);                                                                     \
            if ((want_sums) > 1) p1 = wave_sum(p1);                                                \
            if (lane == 0) {                                                                       \
                red[w] = p0;                                                                       \
                if ((want_sums) > 1) red[RES_WAVES + w] = p1;                                      \
            }                                                                                      \
        }                                                                                          \
        if (dbg) {                                                                                 \
            const long long t_ = __builtin_amdgcn_s_memtime();                                     \
            dbg_acc[4] += t_;                                                                      \
            dbg_acc[5] -= t_;                                                                      \
        }                                                                                          \
        __syncthreads();                                                                           \
        if (dbg) dbg_acc[5] += __builtin_amdgcn_s_memtime();                                       \
        if (want_sums) {                                                                           \
            t0 = res_red8_tree(red);                                                               \
            if ((want_sums) > 1) t1 = res_red8_tree(red + RES_WAVES);                              \
        }                                                                                          \
    } while (0)

    // sum of the LDS vector at `off` over the set bits of `bits` (entry lane + 64 q <-> bit q), n entries
    auto masked_sum = [&](unsigned bits, int off, int n) __attribute__((always_inline)) {
        double s0 = 0.0, s1 = 0.0;
        // (entry lane + 64 q at a constant distance from entry `lane`: one address register and immediate offsets;
        // entries beyond n lie inside the vector's LDS slot -- n <= RES_NMAX / 2 -- and their mask bits are zero)
        (void)n;
        const double* base = sm + off + lane;
        for (int q0 = 0; q0 < 16; q0 += 8) {   // eight gathers in flight (sixteen cost registers the row slices need)
            double x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x[q] = base[64 * (q0 + q)];
            const unsigned bq = bits >> q0;
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                s0 += ((bq >> q) & 1u) ? x[q] : 0.0;
                s1 += ((bq >> (q + 1)) & 1u) ? x[q + 1] : 0.0;
            }
        }
        return wave_sum(s0 + s1);
    };
    double c1 = 0.0, c2s = 0.0;     // kernel-space scalars of the next sweep on level 1 / 2
    // (1'r_2 of the visit: the composed pass now forms it in its finishing lanes and nothing reads this copy, but the
    // encodings of the sweep-form instantiations hang on the store -- without it every one of them is scheduled anew)
    double sumr2p = 0.0;
    (void)sumr2p;
    const double p2ws = POLY2 ? D.p2w[N2] : 0.0;
    double dum0 = 0.0, dum1 = 0.0;
    (void)dum0;
    (void)dum1;

    // r = b - A x (rows of this wave), ||r||, c1 for a zero start; E1 := 0        Class_AMG.m:89,96,103
    // column slices: state of the half sweeps' pipeline.  csFed: the block (0: F, 1: C) whose rows' totals buffer
    // csBuf of PART holds, formed from the values of the last hand-off as they arrived (-1: none).  eFo / eCo: in
    // the finishing lanes (wave 0, lane r < RES_WAVES) the iterate of the workgroup's rows loF + r / loC + r.
    // Every change of an own row's e goes through a publish of that lane, so the lane tracks it in a register
    // (wv + c has the bits of the received v + c that the other threads store) and never reads an entry of E1
    // that another thread may be shifting.
    int csFed = -1, csBuf = 0;
    double eFo = 0.0, eCo = 0.0;
    (void)csFed; (void)csBuf; (void)eFo; (void)eCo;
    // FULL: the post run's last half sweep has added the correction to x, formed the totals of A x and published top's
    // hand-off behind its one barrier (half1_cs); add_correction and top's own row work and publish are then skipped
    bool topfed = false;
    (void)topfed;
    // A times the LDS vector at `off` on both blocks' own rows, one call each: thread t brings entries t, t + BT of
    // the other block.  The caller's barrier follows; then finishing lane 8 sec + r holds row r's total of block sec.
    auto cs_both_rows = [&](int off) __attribute__((always_inline)) {
        const double f0 = tid < nc ? sm[off + nf + tid] : 0.0, f1 = tid + BT < nc ? sm[off + nf + tid + BT] : 0.0;
        const double g0 = tid < nf ? sm[off + tid] : 0.0, g1 = tid + BT < nf ? sm[off + tid + BT] : 0.0;
        res_cs_rows(AF, f0, f1, sm + oPART, w, lane);
        res_cs_rows(AC, g0, g1, sm + oPART + RES_WAVES * RES_WAVES, w, lane);
        csFed = -1;
        eFo = eCo = 0.0;   // (dead outside a run of half sweeps: its first one reloads them)
    };

    // ... after the hand-off's publish barrier, in a publishing lane (wave 0, lane 8 sec + r): b - A v (top) or
    // r - A v of its row, from the eight waves' parts -- published from the register, no trip through oPUB
    auto cs_row_value = [&](int off, bool rhs_b) __attribute__((always_inline)) {
        const bool sec = lane >= RES_WAVES;
        const int r = lane & (RES_WAVES - 1);
        const int row = sec ? RES_OWN_ROW(loC, hiC, r) : RES_OWN_ROW(loF, hiF, r);
        const double T = res_red8_tree(sm + oPART + RES_WAVES * lane);
        const double dg_ = sm[oOWN + (sec ? 3 : 0) * RES_WAVES + r];
        const double base = rhs_b ? sm[oOWN + (sec ? 5 : 2) * RES_WAVES + r] : sm[oR1 + row];
        return base - (T + dg_ * sm[off + row]);
    };

    auto top = [&]() __attribute__((always_inline)) {
        double nrm2 = 0.0, sumr = 0.0;
        bool fed = false;
        if constexpr (FULL) {
            if (topfed) {   // published by the post run's last half sweep: the receipt and its closing barrier remain
                fed = true;
                topfed = false;
                ++seq;
                if (*fail) dead = true;   // (a give-up of that half sweep: its barrier has ordered the flag)
                double hv[4];
                if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
                for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
                if (res_sweep<4>(rs, seq, N1, dead, D.tmo, hv, D.pollsleep)) {
                    *fail = 1;
                    if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (dbg) {
                    const long long t_ = __builtin_amdgcn_s_memtime();
                    dbg_acc[0] += t_;
                    dbg_acc[4] -= t_;
                }
                double p0 = 0.0, p1 = 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = tid + u * BT;
                    const double v = hv[u];
                    sm[oR1 + j] = v;
                    sm[oE1 + j] = 0.0;
                    p0 += v * v;
                    p1 += v;
                }
                p0 = wave_sum(p0);
                p1 = wave_sum(p1);
                if (lane == 0) {
                    red[w] = p0;
                    red[RES_WAVES + w] = p1;
                }
                if (dbg) {
                    const long long t_ = __builtin_amdgcn_s_memtime();
                    dbg_acc[4] += t_;
                    dbg_acc[5] -= t_;
                }
                __syncthreads();
                if (dbg) dbg_acc[5] += __builtin_amdgcn_s_memtime();
                nrm2 = res_red8_tree(red);
                sumr = res_red8_tree(red + RES_WAVES);
            }
        }
        if (!fed) {
        if constexpr (CS1) {
            cls_begin(RES_CL_TOP);
            cs_both_rows(oX);
        } else {
        const double sF = wave_sum(res_rowdot_fma<KR1, 8 * oX>(cF, aF, smb));
        const double sC = wave_sum(res_rowdot_fma<KR1, 8 * oX>(cC, aC, smb));
        if (lane == 0) {
            sm[oPUB + w] = bF - (sF + dgF * sm[oX + rF]);
            sm[oPUB + RES_WAVES + w] = bC - (sC + dgC * sm[oX + rC]);
        }
        }
        if constexpr (CS1)
            RES_HANDOFF_PV(4, N1, loF, hiF - loF, loC, hiC - loC, cs_row_value(oX, true), {},
                           { sm[oR1 + j] = v; sm[oE1 + j] = 0.0; p0 += v * v; p1 += v; }, {}, 2, nrm2, sumr);
        else
        RES_HANDOFF(4, N1, loF, hiF - loF, loC, hiC - loC,
                    { sm[oR1 + j] = v; sm[oE1 + j] = 0.0; p0 += v * v; p1 += v; }, {}, 2, nrm2, sumr);
        }
        c1 = nsp ? sumr * rxx1 : 0.0;
        if constexpr (FULL) {
            // The first half (F rows) of the first pre-smoothing sweep, and the start of the pre run with it: thread t
            // forms entries t and t + BT itself, so they feed the C rows' totals from the registers they were formed
            // in, ahead of the loop's barrier; cycle() publishes the run's first hand-off behind it (no barrier and no
            // trip through E1 of its own).  The finishing lanes form their own rows' entries by the same expression.
            double e0[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = tid + u * BT;
                const double g_i = sm[oR1 + j] - sm[oAX1 + j] * c1;
                e0[u] = sm[oDV1 + j] * g_i;
                sm[oE1 + j] = e0[u];
            }
            csBuf ^= 1;
            res_cs_rows(AC, e0[0], e0[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
            {
                const int row = loF + (lane & (RES_WAVES - 1));
                const double g_i = sm[oR1 + row] - sm[oAX1 + row] * c1;
                eFo = sm[oDV1 + row] * g_i;
                eCo = 0.0;
            }
            csFed = 1;
            __syncthreads();
        } else
        if (lfirst) {   // first half (F rows) of the first pre-smoothing sweep: half1(true, true, true)
            for (int j = tid; j < nf; j += BT) {
                const double g_i = sm[oR1 + j] - sm[oAX1 + j] * c1;
                sm[oE1 + j] = sm[oDV1 + j] * g_i;
            }
            __syncthreads();
        }
        cls_end(RES_CL_TOP);
        return sqrt(nrm2);
    };

    // one half of a bigraph Gauss-Seidel sweep on level 1.  `first`: rows of the first half (the
    // other half still holds the old iterate); second half: + the shift by c of both halves and
    // the scalar of the next sweep.                         MG_Vcycle.m:15-21,34-38; Class_AMG.m:56-59
    //
    // Column slices: ONE barrier per half sweep.  The values of block X that a thread has just received are
    // multiplied, in the registers they arrived in, with the workgroup's rows of the other block (whose columns
    // X are), reduced by res_cs_rows and left in PART before the barrier; after it the finishing lanes add the
    // eight waves' parts, finish their rows and publish the NEXT half sweep from registers.  Whatever else the
    // step needs (the other half's shift by c and its part of the next scalar, the reads of r and A*1) runs
    // between that publish and the next wait.  `feed`: the next hand-off is the other block's half sweep.  A
    // half sweep that does not follow the other block's (the first of a run) takes its totals from E1 in LDS
    // first, with a barrier of its own.
    // the finishing lanes (wave 0, lane r < RES_WAVES) of hand-off `sq`: row totals -> new values -> publish
    auto cs_finish = [&](bool frows, bool first, bool zs, unsigned sq) __attribute__((always_inline)) {
        if (dbg) dbg_acc[8] -= __builtin_amdgcn_s_memtime();
        const double cc = c1;
        if (w == 0 && lane < RES_WAVES) {
            // (every workgroup owns a row of every block)
            const int row = frows ? RES_OWN_ROW(loF, hiF, lane) : RES_OWN_ROW(loC, hiC, lane);
            const int g0 = frows ? loF : loC - nf, cnt = frows ? hiF - loF : hiC - loC;
            // (the row's own scalars first: their reads go out with the parts', one LDS latency for all)
            const double dg_ = sm[oOWN + (frows ? 0 : 3) * RES_WAVES + lane];
            const double dv_ = sm[oOWN + (frows ? 1 : 4) * RES_WAVES + lane];
            const double r_own = sm[oR1 + row], ax_own = sm[oAX1 + row];
            const double T = zs ? 0.0 : res_red8_tree(sm + oPART + RES_WAVES * RES_WAVES * csBuf + RES_WAVES * lane);
            const double eo = frows ? eFo : eCo;
            const double s = T + dg_ * eo;
            const double g_i = r_own - s - ax_own * cc;
            const double wv = eo + dv_ * g_i;
            if (lane < cnt && !RES_SKIPPED(sq)) res_publish(rs, sq, g0 + lane, wv);
            // this half: wv (+ c in a second half); the other half: + c in a second half
            const double mine = first ? wv : wv + cc;
            if (frows) {
                eFo = mine;
                if (!first) eCo = eCo + cc;
            } else {
                eCo = mine;
                if (!first) eFo = eFo + cc;
            }
        }
        if (dbg) dbg_acc[8] += __builtin_amdgcn_s_memtime();
    };
    // `start`: the first hand-off of a run (csFed != me), for the stamps by class
    auto half1_cs = [&](bool frows, bool first, bool ezero, bool feed, bool start) __attribute__((always_inline)) {
        const int blk0 = frows ? 0 : nf, nblk = frows ? nf : nc;
        const int oth0 = frows ? nf : 0, noth = frows ? nc : nf;
        const int me = frows ? 0 : 1;
        if constexpr (FULL) {
            if (!feed) {
                // The last half sweep of a run (a second half, published behind the barrier of the half sweep before
                // it) carries the hand-off that follows the run: rr = r - A e behind the pre run (C rows), top's
                // r = b - A x behind the post run (F rows), whose vector is then x + e: add_correction's own add, made
                // here by the thread that holds the entry.  Both blocks' totals of A times that vector are formed on
                // the way: the other block's entries, shifted by c between the publish and the wait, are the columns
                // of this block's rows (totals in buffer PART3); the received entries are the columns of the other
                // block's rows (totals in buffer csBuf ^ 1, at the receipt).  Behind the one barrier the finishing
                // lanes finish the rows and publish from registers: cs_both_rows' pass and the publish barrier of the
                // hand-off are gone.  Nothing reads c1 before that hand-off sets it again (the prolongation's receipt
                // or top's), so no part of the scalar is formed either.
                cls_begin(RES_CL_HALF);
                ++seq;
                if (*fail) dead = true;
                const double cc = c1;
                double ov[2], xo[2] = {0.0, 0.0}, hv[2] = {0.0, 0.0}, mv[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {   // (each entry of E1 and of X is read and written by thread j % BT alone)
                    const int jo = oth0 + tid + u * BT;
                    const double en = sm[oE1 + jo] + cc;
                    sm[oE1 + jo] = en;
                    if (frows) {
                        const double xn = sm[oX + jo] + en;
                        sm[oX + jo] = xn;
                        ov[u] = xn;
                        xo[u] = sm[oX + blk0 + tid + u * BT];
                    } else {
                        ov[u] = en;
                    }
                }
                if (frows)
                    res_cs_rows(AF, ov[0], ov[1], sm + oPART3, w, lane);
                else
                    res_cs_rows(AC, ov[0], ov[1], sm + oPART3, w, lane);
                if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
                for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
                if (res_sweep<2>(rs, seq, nblk, dead, D.tmo, hv, D.pollsleep)) {
                    *fail = 1;
                    if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (dbg) {
                    const long long t_ = __builtin_amdgcn_s_memtime();
                    dbg_acc[0] += t_;
                    dbg_acc[4] -= t_;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int j = blk0 + tid + u * BT;
                    const double en = hv[u] + cc;
                    sm[oE1 + j] = en;
                    if (frows) {
                        const double xn = xo[u] + en;
                        sm[oX + j] = xn;
                        mv[u] = xn;
                    } else {
                        mv[u] = en;
                    }
                }
                csBuf ^= 1;
                if (frows)
                    res_cs_rows(AC, mv[0], mv[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
                else
                    res_cs_rows(AF, mv[0], mv[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
                if (dbg) {
                    const long long t_ = __builtin_amdgcn_s_memtime();
                    dbg_acc[4] += t_;
                    dbg_acc[3] -= t_;
                }
                __syncthreads();
                if (dbg) dbg_acc[3] += __builtin_amdgcn_s_memtime();
                cls_end(RES_CL_HALF);
                cls_begin(frows ? RES_CL_TOP : RES_CL_RR);
                // finishing lanes: the F rows' totals lie where this block's or the other block's went
                const double* totF = frows ? sm + oPART3 : sm + oPART + RES_WAVES * RES_WAVES * csBuf;
                const double* totC = frows ? sm + oPART + RES_WAVES * RES_WAVES * csBuf : sm + oPART3;
                if (frows) {   // top: b - (A x) of both blocks' rows, 2 RES_WAVES granules (cs_row_value(oX, true))
                    if (w == 0 && lane < 2 * RES_WAVES) {
                        const bool sec = lane >= RES_WAVES;
                        const int r = lane & (RES_WAVES - 1);
                        const int row = (sec ? loC : loF) + r;
                        const double T = res_red8_tree((sec ? totC : totF) + RES_WAVES * r);
                        const double dg_ = sm[oOWN + (sec ? 3 : 0) * RES_WAVES + r];
                        const double base = sm[oOWN + (sec ? 5 : 2) * RES_WAVES + r];
                        const double val = base - (T + dg_ * sm[oX + row]);
                        if (!RES_SKIPPED(seq + 1)) res_publish(rs, seq + 1, row, val);
                    }
                    topfed = true;
                } else {       // rr: the F block is published, the own C rows' entries stay in the workgroup
                    if (w == 0 && lane < RES_WAVES) {
                        const double TF = res_red8_tree(totF + RES_WAVES * lane);
                        const double TC = res_red8_tree(totC + RES_WAVES * lane);
                        const double dF_ = sm[oOWN + 0 * RES_WAVES + lane], dC_ = sm[oOWN + 3 * RES_WAVES + lane];
                        const double rF_ = sm[oR1 + loF + lane], rC_ = sm[oR1 + loC + lane];
                        const double val = rF_ - (TF + dF_ * eFo);
                        if (!RES_SKIPPED(seq + 1)) res_publish(rs, seq + 1, loF + lane, val);
                        sm[oRR1 + loC + lane] = rC_ - (TC + dC_ * eCo);
                    }
                }
                csFed = -1;
                eFo = eCo = 0.0;   // (dead outside a run of half sweeps)
                return;
            }
        }
        cls_begin(start ? RES_CL_START : RES_CL_HALF);
        ++seq;
        if (*fail) dead = true;           // (a give-up of the previous hand-off: its barrier has ordered the flag)
        if (ezero && first) {             // zero start: the row's sum and its own entry are zero
            eFo = eCo = 0.0;
            cs_finish(frows, first, true, seq);
        } else if (!FULL && csFed != me) {   // the first of a run: the totals from E1 in LDS, the own entries too (FULL: every run is fed)
            const double v0 = tid < noth ? sm[oE1 + oth0 + tid] : 0.0;
            const double v1 = tid + BT < noth ? sm[oE1 + oth0 + tid + BT] : 0.0;
            csBuf ^= 1;
            if (frows)
                res_cs_rows(AF, v0, v1, sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
            else
                res_cs_rows(AC, v0, v1, sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
            eFo = sm[oE1 + RES_OWN_ROW(loF, hiF, lane)];
            eCo = sm[oE1 + RES_OWN_ROW(loC, hiC, lane)];
            __syncthreads();
            cs_finish(frows, first, false, seq);
        }
        // (else: published behind the barrier of the other block's half sweep, below)
        // ---- between the publish and the wait ------------------------------------------------------------
        const double cc = c1;
        double pa[2] = {0.0, 0.0}, pb[2] = {0.0, 0.0}, p0 = 0.0;
        if (!first) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int j = tid + u * BT;
                if (j < nblk) {
                    pa[u] = sm[oR1 + blk0 + j];
                    pb[u] = sm[oAX1 + blk0 + j];
                }
            }
            // other half: w -> w + c, and its part of the scalar of the next sweep (each entry of E1 is read and
            // written by thread j % BT alone, here, in the receipt below and in the reads that feed res_cs_rows)
            for (int jo = tid; jo < noth; jo += BT) {
                const double en = sm[oE1 + oth0 + jo] + cc;
                sm[oE1 + oth0 + jo] = en;
                p0 += sm[oR1 + oth0 + jo] - sm[oAX1 + oth0 + jo] * en;
            }
        }
        if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
        for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
        double hv[2] = {0.0, 0.0};
        if (res_sweep<2>(rs, seq, nblk, dead, D.tmo, hv, D.pollsleep)) {
            *fail = 1;
            if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (dbg) {
            const long long t_ = __builtin_amdgcn_s_memtime();
            dbg_acc[0] += t_;
            dbg_acc[4] -= t_;
        }
        // ---- receipt: the values meet their matrix entries in the registers they arrived in ---------------
        double en[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = tid + u * BT;
            en[u] = j < nblk ? (first ? hv[u] : hv[u] + cc) : 0.0;
        }
        if (feed) {
            csBuf ^= 1;
            if (frows)
                res_cs_rows(AC, en[0], en[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
            else
                res_cs_rows(AF, en[0], en[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
            csFed = 1 - me;
        } else {
            csFed = -1;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = tid + u * BT;
            if (j < nblk) {
                sm[oE1 + blk0 + j] = en[u];
                if (!first) p0 += pa[u] - pb[u] * en[u];
            }
        }
        double* part9 = sm + oPART9 + RES_WAVES * (int)(seq & 1);
        if (!first && nsp) {
            p0 = wave_sum(p0);
            if (lane == 0) part9[w] = p0;
        }
        if (dbg) {
            const long long t_ = __builtin_amdgcn_s_memtime();
            dbg_acc[4] += t_;
            dbg_acc[3] -= t_;
        }
        __syncthreads();
        if (dbg) dbg_acc[3] += __builtin_amdgcn_s_memtime();
        // the scalar of the next sweep and, where the other block's half sweep follows, its publish: the reads of
        // the waves' parts, of the scalar's parts and of the rows' own scalars go out together
        if (!first) c1 = nsp ? res_red8_tree(part9) * rxx1 : 0.0;
        if (feed)
            cs_finish(!frows, !first, false, seq + 1);
        else
            eFo = eCo = 0.0;   // (dead outside a run of half sweeps: its first one reloads them)
        cls_end(start ? RES_CL_START : RES_CL_HALF);
    };
    auto half1 = [&](bool frows, bool first, bool ezero) __attribute__((always_inline)) {
        if constexpr (!CS1) {   // (16-entry rows: half1_cs)
        double s = 0.0, eo = 0.0;
        const int row = frows ? rowF : rowC;
        const bool valid = frows ? vF : vC;
        const int rr_ = valid ? row : 0;
        // the row's own scalars first: their LDS round trips overlap the gathers of the row (read after the
        // wave sum they were one more dependent LDS latency on every half sweep's critical path)
        if (!ezero) eo = sm[oE1 + rr_];
        const double dg_ = frows ? dgF : dgC, dv_ = frows ? dvF : dvC;
        const double r_own = sm[oR1 + rr_], ax_own = sm[oAX1 + rr_];
        if (!(ezero && first)) s = wave_sum(frows ? res_rowdot_fma<KR1, 8 * oE1>(cF, aF, smb) : res_rowdot_fma<KR1, 8 * oE1>(cC, aC, smb));
        s += dg_ * eo;
        const double g_i = r_own - s - ax_own * c1;
        const double wv = eo + dv_ * g_i;
        const int blk0 = frows ? 0 : nf, nblk = frows ? nf : nc;
        if (lane == 0) sm[oPUB + w] = wv;
        const int g0 = (frows ? loF : loC) - blk0, cnt = frows ? hiF - loF : hiC - loC;
        if (first) {
            RES_HANDOFF(2, nblk, g0, cnt, 0, 0, { sm[oE1 + blk0 + j] = v; }, {}, 0, dum0, dum1);
        } else {
            // other half: w -> w + c ; this half: wv + c ; scalar of the next sweep
            const int oth0 = frows ? nf : 0, noth = frows ? nc : nf;
            const double cc = c1;
            double xig = 0.0;
            RES_HANDOFF_P(2, nblk, g0, cnt, 0, 0,
                          { pa_[u_] = sm[oR1 + blk0 + j]; pb_[u_] = sm[oAX1 + blk0 + j]; },
                          {
                              const double en = v + cc;
                              sm[oE1 + blk0 + j] = en;
                              p0 += pa_[u_] - pb_[u_] * en;
                          },
                          {
                              for (int jo = tid; jo < noth; jo += BT) {
                                  const double en = sm[oE1 + oth0 + jo] + cc;
                                  sm[oE1 + oth0 + jo] = en;
                                  p0 += sm[oR1 + oth0 + jo] - sm[oAX1 + oth0 + jo] * en;
                              }
                          },
                          (nsp ? 1 : 0), xig, dum1);
            c1 = nsp ? xig * rxx1 : 0.0;
        }
        }
    };
    auto sweep1 = [&](bool post, bool ezero, bool last, bool start) __attribute__((always_inline)) {
        (void)start;
        if constexpr (CS1) {
            const bool local = lfirst && ezero && !post;   // (the first half: done by top())
            if (!local) half1_cs(!post, true, ezero, true, start);
            half1_cs(post, false, ezero, !last, FULL ? false : local);   // (the run's next sweep starts with the other block; FULL: top() has fed the start)
        } else {
        if (!(lfirst && ezero && !post)) half1(!post, true, ezero);   // else: done by top()    // pre: F rows first (Rk{1}); post: C rows first (Rk{1}')
        half1(post, false, ezero);
        }
    };

    // weighted-Jacobi sweep on level 2                                   MG_Vcycle.m:15-21; Class_AMG.m:84
    auto sweep2 = [&](bool ezero) __attribute__((always_inline)) {
        cls_begin(RES_CL_LEVEL2);
        double s = 0.0, eo = 0.0;
        if (!ezero) {
            s = wave_sum(res_rowdot_fma<KE2, 8 * oE2>(c2, a2, smb));
            eo = sm[oE2 + r2];
            s += dg2 * eo;
        }
        const double g_i = sm[oR2 + r2] - s - sm[oAX2 + r2] * c2s;
        const double wv = eo + dv2 * g_i;
        if (lane == 0) sm[oPUB + w] = wv;
        const double cc = c2s;
        double xig = 0.0;
        RES_HANDOFF_P(4, N2, lo2, hi2 - lo2, 0, 0, { pa_[u_] = sm[oR2 + j]; pb_[u_] = sm[oAX2 + j]; },
                      {
                          const double en = v + cc;
                          sm[oE2 + j] = en;
                          p0 += pa_[u_] - pb_[u_] * en;
                      },
                      {}, (nsp ? 1 : 0), xig, dum1);
        c2s = nsp ? xig * rxx2 : 0.0;
        cls_end(RES_CL_LEVEL2);
    };

    // tail level: restriction, Jacobi-PCG (PCG.m:68-87, zero guess), prolongation -- all of it by
    // every workgroup on its own LDS copies, so no hand-off                     MG_Vcycle.m:27-31,43
    const auto rtin = __builtin_amdgcn_make_buffer_rsrc(D.tail.tin, 0, 2 * RES_GRAN_MAX * 16, 0x00020000);
    const auto rtout = __builtin_amdgcn_make_buffer_rsrc(D.tail.tout, 0, 2 * RES_GRAN_MAX * 16, 0x00020000);
    unsigned tseq = 0;      // number of the last visit of the remote tail
    // Remote tail: the residual of the level above the tail's root (LDS offset oRRs) is restricted row
    // by row -- row i of the restriction by wave i / G of workgroup i % G (Nt <= BT <= 8 G rows) --
    // straight into the tail workgroup's inbox; then everybody waits for the prolongated correction
    // (Nout granules) and finishes e += P e_tail on its copy (offsets oEd, oRd, oAXd), with the scalar
    // of the next sweep.
    auto remote_tail = [&](const ResCsr& Pin, int oRRs, int oEd, int oRd, int oAXd, double xxd, int Nout,
                           double& cnext) __attribute__((always_inline)) {
        ++tseq;
        const int rin = b + G * w;
        if (rin < Nt) {
            const double s3 = res_csr_rowdot(Pin, rowp[12 * w + 6], rowp[12 * w + 7], lane, sm, oRRs);
            if (lane == 0) res_tail_post(rtin, tseq, rin, s3);
        }
        double hv[4];
        const int st = res_tail_wait<4>(rtout, tseq, Nout, D.tmo, fail, dead, lane, hv);
        double p0 = 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = tid + u * BT;
            if (j < Nout && !dead && !st) {
                const double en = sm[oEd + j] + hv[u];
                sm[oEd + j] = en;
                p0 += sm[oRd + j] - sm[oAXd + j] * en;
            }
        }
        if (nsp) {
            p0 = wave_sum(p0);
            if (lane == 0) red[w] = p0;
        }
        __syncthreads();
        if (nsp) cnext = res_red8(red) / xxd;
        if (*fail) dead = true;
    };
    // Local tail (at most 64 rows, solved redundantly by every workgroup on its own LDS copies, so no
    // hand-off): restriction of the level above (residual at oRRs), Jacobi-PCG (PCG.m:68-87, zero
    // guess), prolongation into the level above (oEd, with oRd / oAXd for the next scalar).
    auto local_tail = [&](const ResCsr& PtT, const ResCsr& AT, const ResCsr& PT, int oRRs, int oEd, int oRd,
                          int oAXd, double xxd, int Nabove, double& cnext) __attribute__((always_inline)) {
        if (Nt == 1) {
            // one row: its entries are dealt to all the waves, the eight partial sums are added in
            // wave order (a single wave walking 1024 entries took four dependent trips)
            const int e0 = PtT.rp[0], e1 = PtT.rp[1];
            double s = 0.0;
            for (int t = e0 + tid; t < e1; t += BT * 2) {
                const int t1 = t + BT;
                const int ja = PtT.ci[t], jb = PtT.ci[t1 < e1 ? t1 : e0];
                const double aa = PtT.va[t], ab = PtT.va[t1 < e1 ? t1 : e0];
                s += aa * sm[oRRs + ja];
                s += t1 < e1 ? ab * sm[oRRs + jb] : 0.0;
            }
            s = wave_sum(s);
            if (lane == 0) red[w] = s;
            __syncthreads();
            if (tid == 0) sm[oR3] = res_red8(red);
        } else {
            for (int i = w; i < Nt; i += RES_WAVES) {
                const double s = res_csr_rowdot(PtT, PtT.rp[i], PtT.rp[i + 1], lane, sm, oRRs);
                if (lane == 0) sm[oR3 + i] = s;
            }
        }
        __syncthreads();
        if (w == 0) {
            const int i = lane < Nt ? lane : 0;
            const bool valid = lane < Nt;
            const int e0 = AT.rp[i], e1 = AT.rp[i + 1];
            double dd = 0.0;
            for (int t = e0; t < e1; ++t)
                if (AT.ci[t] == i) dd = AT.va[t];
            double r = valid ? sm[oR3 + i] : 0.0;
            double p = valid ? r / dd : 0.0;
            double d = 0.0;
            double delta_new = wave_sum(valid ? r * p : 0.0);
            const double thresh = 1e-11 * 1e-11 * delta_new;
            long long it = 0;
            while (it < D.pcg_maxit && delta_new > thresh) {
                const double delta_old = delta_new;
                if (valid) sm[oP3 + i] = p;
                tiny_sync();
                double q = 0.0;
                if (valid)
                    for (int t = e0; t < e1; ++t) q += AT.va[t] * sm[oP3 + AT.ci[t]];
                tiny_sync();
                const double qp = wave_sum(valid ? q * p : 0.0);
                const double alpha = delta_old / qp;
                d += alpha * p;
                r = r - alpha * q;
                const double wi = valid ? r / dd : 0.0;
                delta_new = wave_sum(valid ? r * wi : 0.0);
                p = wi + (delta_new / delta_old) * p;
                ++it;
            }
            if (valid) sm[oE3 + i] = d;
        }
        __syncthreads();
        double p0 = 0.0;
        for (int j = tid; j < Nabove; j += BT) {
            double s = 0.0;
            for (int t = PT.rp[j]; t < PT.rp[j + 1]; ++t) s += PT.va[t] * sm[oE3 + PT.ci[t]];
            const double en = sm[oEd + j] + s;
            sm[oEd + j] = en;
            p0 += sm[oRd + j] - sm[oAXd + j] * en;
        }
        if (nsp) {
            p0 = wave_sum(p0);
            if (lane == 0) red[w] = p0;
        }
        __syncthreads();
        if (nsp) cnext = res_red8(red) / xxd;
        };
    auto tail = [&]() __attribute__((always_inline)) {
        if (RES_REMOTE) {
            remote_tail(D.Pt3, oRR2, oE2, oR2, oAX2, xx2, N2, c2s);
            return;
        }
        if (tail1) {
            double s = 0.0;
            for (int j = tid; j < N2; j += BT) s += sm[oP3C + j] * sm[oRR2 + j];       // r_3 = P' rr
            s = wave_sum(s);
            if (lane == 0) red[w] = s;
            __syncthreads();
            const double d = res_pcg_1x1(res_red8(red), h33, D.pcg_maxit);
            __syncthreads();   // red is rewritten below
            double p0 = 0.0;
            for (int j = tid; j < N2; j += BT) {                                       // e_2 += P e_3
                const double en = sm[oE2 + j] + sm[oP3C + j] * d;
                sm[oE2 + j] = en;
                p0 += sm[oR2 + j] - sm[oAX2 + j] * en;
            }
            if (nsp) {
                p0 = wave_sum(p0);
                if (lane == 0) red[w] = p0;
            }
            __syncthreads();
            if (nsp) c2s = res_red8(red) / xx2;
            return;
        }
        local_tail(D.Pt3, D.A3, D.P3, oRR2, oE2, oR2, oAX2, xx2, N2, c2s);
    };

    // ---- third resident level (THREE): Jacobi like level 2, N3 <= BT rows dealt in contiguous runs to the
    // workgroups (0-4 rows each).  A workgroup without a row still has to say that it has finished a
    // step (the two-buffer protocol lets a buffer be rewritten once everybody has published the step in
    // between), so every workgroup publishes one extra "ack" granule, N3 + b, with its rows.
    double c3s = 0.0, sumr3 = 0.0;
#define RES_HANDOFF3(STORE3, want_sums, t0)                                                              \
    do {                                                                                                 \
        if (w == 0 && lane == 0) sm[oPUB + RES_WAVES] = 0.0;                                             \
        RES_HANDOFF(2, N3 + G, lo3, hi3 - lo3, N3 + b, 1, { if (j < N3) { STORE3; } }, {}, want_sums, t0, dum1); \
    } while (0)
    // POLY4: the ack granule of workgroup b < N4 carries r_4[b] (the restricted residual goes to everybody) ...
#define RES_HANDOFF3R(ACKV, STORE3, STORE4, want_sums, t0)                                               \
    do {                                                                                                 \
        if (w == 0 && lane == 0) sm[oPUB + RES_WAVES] = (ACKV);                                          \
        RES_HANDOFF(2, N3 + G, lo3, hi3 - lo3, N3 + b, 1,                                                \
                    { if (j < N3) { STORE3; } else if (j - N3 < Nt) { const int j4 = j - N3; STORE4; } }, {}, want_sums, t0, dum1); \
    } while (0)
    // ... and the hand-off among the rows of level 4: row b of workgroup b < N4, an ack granule of everybody
#define RES_HANDOFF4(STORE4)                                                                             \
    do {                                                                                                 \
        if (w == 0 && lane == 0) sm[oPUB + RES_WAVES] = 0.0;                                             \
        RES_HANDOFF(1, Nt + G, b, (b < Nt ? 1 : 0), Nt + b, 1, { if (j < Nt) { STORE4; } }, {}, 0, dum0, dum1); \
    } while (0)
    auto sweep3 = [&](bool ezero) __attribute__((always_inline)) {
        if (THREE) {
            double s = 0.0, eo = 0.0;
            if (!ezero) {
                s = wave_sum(res_rowdot<K3, 8 * oE3L>(c3, a3, smb));
                eo = sm[oE3L + r3];
                s += dg3 * eo;
            }
            const double g_i = sm[oR3L + r3] - s - sm[oAX3L + r3] * c3s;
            const double wv = eo + dv3 * g_i;
            if (lane == 0) sm[oPUB + w] = wv;
            const double cc = c3s;
            double xig = 0.0;
            RES_HANDOFF3({
                             const double en = v + cc;
                             sm[oE3L + j] = en;
                             p0 += sm[oR3L + j] - sm[oAX3L + j] * en;
                         },
                         (nsp ? 1 : 0), xig);
            c3s = nsp ? xig * rxx3 : 0.0;
        }
    };
    // one visit of level 3 and, through the remote tail rooted at level 4, of everything below it
    // polynomial form: the sums of this workgroup's rows against [r_3; e_3] (+ their factor of 1'r_3)
    // -> sm[oR3 + 40 + q]; the caller's next barrier publishes them
    auto poly3_rows = [&](int nrows, bool post) __attribute__((always_inline)) {
        const double xr = tid < N3 ? sm[oR3L + tid] : 0.0, xe = tid < N3 ? sm[oE3L + tid] : 0.0;
        const double xc = (post && tid < Nt) ? sm[oRR3L + tid] : 0.0;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            if (q < nrows) {
                double t = __builtin_fma(m3e[q], xe, m3r[q] * xr);
                if (q < 4) t = __builtin_fma(m3c[q], xc, t);
                const double pq = wave_sum(t);
                if (lane == 0) sm[oR3 + 8 * q + w] = pq;
            }
        }
        __syncthreads();
        if (tid < nrows) {
            double sq = 0.0;
#pragma unroll
            for (int ww = 0; ww < RES_WAVES; ++ww) sq += sm[oR3 + 8 * tid + ww];
            sm[oR3 + 40 + tid] = __builtin_fma(sm[oE3 + tid], sumr3, sq);
        }
        __syncthreads();
    };
    // POLY4: workgroup b's row of level 4 (b < N4 = Nt) and restriction row N4 + b (b < N5) against [r_4; e_4]
    // (+ (M1 P5) e_5 in the second pass) -> sm[oPS4 + 16 + q]; coefficients from L2 at every pass, one entry per
    // thread and segment (threads 0..127).  e_4 lives where the tail's answer of the POLY3 mode does (oRR3L).
    const int N5 = POLY3 ? D.N5 : 0;
    const bool poly4 = POLY3 && N5 > 0;
    double sumr4 = 0.0;
    auto poly4_rows = [&](int nrows, bool post) __attribute__((always_inline)) {
        // rows q = 0: row b of [M2a | M1] (b < N4), q = 1: restriction row N4 + b (b < N5; first pass only)
        double m4r[2], m4e[2], m4c;
        const int t4 = tid < RES_P4_SEG ? tid : 0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int row = q == 0 ? b : Nt + b;
            const bool okr = q < nrows && (q == 0 ? b < Nt : b < N5) && tid < RES_P4_SEG;
            const double* pr = D.p4rows + (size_t)(okr ? row : 0) * RES_P4_LD;
            const double vr = pr[t4], ve = pr[RES_P4_SEG + t4];
            m4r[q] = okr ? vr : 0.0;
            m4e[q] = okr ? ve : 0.0;
            if (q == 0) {
                const double vc = pr[2 * RES_P4_SEG + (tid < 64 ? tid : 0)];
                m4c = (okr && post && tid < N5) ? vc : 0.0;
            }
        }
        const double xr = tid < Nt ? sm[oR4L + t4] : 0.0, xe = tid < Nt ? sm[oRR3L + t4] : 0.0;
        const double xc = (post && tid < N5) ? sm[oE5L + tid] : 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (q < nrows) {
                double t = __builtin_fma(m4e[q], xe, m4r[q] * xr);
                if (q == 0) t = __builtin_fma(m4c, xc, t);
                const double pq = wave_sum(t);
                if (lane == 0) sm[oPS4 + 8 * q + w] = pq;
            }
        }
        __syncthreads();
        if (tid < nrows) {
            double sq = 0.0;
#pragma unroll
            for (int ww = 0; ww < RES_WAVES; ++ww) sq += sm[oPS4 + 8 * tid + ww];
            sm[oPS4 + 16 + tid] = __builtin_fma(sm[oPS4 + 20 + tid], sumr4, sq);
        }
        __syncthreads();
    };
    auto visit3 = [&](bool keep) __attribute__((always_inline)) {
        if (POLY3) {
            // e' = M2a r + M1 e and the restricted residual of e' in one pass                 MG_Vcycle.m:20-29
            poly3_rows(5, false);
            if (poly4) {   // r_4 to everybody (ack granules), e_4 := 0; then level 4's own visits      MG_Wcycle.m:28-30
                if (tid < 4) sm[oPUB + tid] = sm[oR3 + 40 + tid];
                double s4 = 0.0;
                RES_HANDOFF3R((b < Nt ? sm[oR3 + 44] : 0.0), { sm[oE3L + j] = v; },
                              { sm[oR4L + j4] = v; sm[oRR3L + j4] = 0.0; p0 += v; }, (nsp ? 1 : 0), s4);
                sumr4 = nsp ? s4 : 0.0;
                for (int leg = 0; leg < (D.wcycle ? 2 : 1); ++leg) {
                    ++tseq;
                    poly4_rows(2, false);                              // e_4' (row b) and r_5[b] = P5'(r_4 - A_4 e_4')
                    if (tid == 0 && b < N5) res_tail_post(rtin, tseq, b, sm[oPS4 + 17]);
                    if (tid == 0) sm[oPUB] = sm[oPS4 + 16];
                    RES_HANDOFF4({ sm[oRR3L + j] = v; });
                    res_tail_answer<1>(rtout, tseq, N5, D.tmo, fail, dead, sm, oE5L, tid, lane);   // e_5
                    poly4_rows(1, true);                               // e_4'' = M2a r + M1 e' + (M1 P5) e_5
                    if (tid == 0) sm[oPUB] = sm[oPS4 + 16];
                    RES_HANDOFF4({ sm[oRR3L + j] = v; });
                }
            } else {
                ++tseq;
                if (tid == 0 && b < Nt) res_tail_post(rtin, tseq, b, sm[oR3 + 44]);
                if (tid < 4) sm[oPUB + tid] = sm[oR3 + 40 + tid];
                RES_HANDOFF3({ sm[oE3L + j] = v; }, 0, dum0);
                res_tail_answer<1>(rtout, tseq, Nt, D.tmo, fail, dead, sm, oRR3L, tid, lane);   // e_4 (Nt <= G <= BT values)
            }
            poly3_rows(4, true);                                         // e'' = M2a r + M1 e' + (M1 P4) e_4   :31-41
            if (tid < 4) sm[oPUB + tid] = sm[oR3 + 40 + tid];
            RES_HANDOFF3({ sm[oE3L + j] = v; }, 0, dum0);
            (void)keep;
        } else if (THREE) {
            const int nu = D.nu;
            for (int s = 0; s < nu; ++s) sweep3(!keep && s == 0);
            {   // rr = r - A e                                                       MG_Vcycle.m:27
                const double s = wave_sum(res_rowdot<K3, 8 * oE3L>(c3, a3, smb)) + dg3 * sm[oE3L + r3];
                if (lane == 0) sm[oPUB + w] = sm[oR3L + r3] - s;
                RES_HANDOFF3({ sm[oRR3L + j] = v; }, 0, dum0);
            }
            if (RES_REMOTE)
                remote_tail(D.Pt4, oRR3L, oE3L, oR3L, oAX3L, xx3, N3, c3s);
            else
                local_tail(D.Pt4, D.A4, D.P4, oRR3L, oE3L, oR3L, oAX3L, xx3, N3, c3s);
            for (int s = 0; s < nu; ++s) sweep3(false);
        }
    };

    // one visit of level 2 and everything below it
    auto visit2 = [&](bool keep) __attribute__((always_inline)) {
        const int nu = D.nu;
        for (int s = (lfirst2 && !keep) ? 1 : 0; s < nu; ++s) sweep2(!keep && s == 0);
        // rr = r - A e                                                           MG_Vcycle.m:27
        {
            cls_begin(RES_CL_LEVEL2);
            const double s = wave_sum(res_rowdot_fma<KE2, 8 * oE2>(c2, a2, smb)) + dg2 * sm[oE2 + r2];
            if (lane == 0) sm[oPUB + w] = sm[oR2 + r2] - s;
            RES_HANDOFF(4, N2, lo2, hi2 - lo2, 0, 0, { sm[oRR2 + j] = v; }, {}, 0, dum0, dum1);
        }
        if (dbg) dbg_acc[7] -= __builtin_amdgcn_s_memtime();
        if (THREE) {
            {   // r_3 = P3' rr_2 ; E3 := 0 ; c for the zero start
                const double s = res_csr_rowdot(D.Pt3, rowp[12 * w + 8], rowp[12 * w + 9], lane, sm, oRR2);
                if (lane == 0) sm[oPUB + w] = s;
                double sumr = 0.0;
                RES_HANDOFF3({ sm[oR3L + j] = v; sm[oE3L + j] = 0.0; p0 += v; }, (nsp ? 1 : 0), sumr);
                c3s = nsp ? sumr * rxx3 : 0.0;
                sumr3 = sumr;
            }
            for (int leg = 0; leg < (D.wcycle ? 2 : 1); ++leg) visit3(leg == 1);   // MG_Wcycle.m:28-30
            {   // e_2 += P3 e_3                                                     MG_Vcycle.m:31
                const double sP = res_csr_rowdot(D.P3, rowp[12 * w + 10], rowp[12 * w + 11], lane, sm, oE3L);
                if (lane == 0) sm[oPUB + w] = sm[oE2 + r2] + sP;
                double xig = 0.0;
                RES_HANDOFF_P(4, N2, lo2, hi2 - lo2, 0, 0, { pa_[u_] = sm[oR2 + j]; pb_[u_] = sm[oAX2 + j]; },
                              { sm[oE2 + j] = v; p0 += pa_[u_] - pb_[u_] * v; }, {}, (nsp ? 1 : 0), xig, dum1);
                c2s = nsp ? xig * rxx2 : 0.0;
            }
        } else {
            tail();
        }
        if (dbg) dbg_acc[7] += __builtin_amdgcn_s_memtime();
        cls_end(RES_CL_LEVEL2);   // (the residual's hand-off, with the tail behind it)
        for (int s = 0; s < nu; ++s) sweep2(false);
    };

    // Level 2 composed over a visit (POLY2), fed from the polls of r_2: r_2's hand-off is published from oPUB like any
    // other, and what arrives meets the column slices of B in the registers it arrived in.  res_cs_rows leaves the
    // waves' row totals in PART, the waves' parts of s'r_2 and 1'r_2 go to red, and after ONE barrier the finishing
    // lanes (wave 0, lane r < RES_WAVES) hold all of
    //     e_2 = B r_2 + wB (1'r_2) + mp e_3,   e_3 = PCG(h33, s'r_2 + ws (1'r_2))            (PCG.m:68-87, one row)
    // for their rows: they publish e_2's hand-off from registers, and its receipt is the visit's only LDS store.
    // Nothing reads r_2 afterwards, so it is not kept.  (PART and red are free here: the hand-offs on either side
    // have a barrier between their use of them and this one.)
    auto poly2_fed = [&]() __attribute__((always_inline)) {
        if constexpr (POLY2) {
            ++seq;
            if (*fail) dead = true;
            if (dbg) dbg_acc[3] -= __builtin_amdgcn_s_memtime();
            __syncthreads();
            if (dbg) dbg_acc[3] += __builtin_amdgcn_s_memtime();
            const bool pub = w == 0 && lane < RES_WAVES && lane < hi2 - lo2;
            if (pub && !RES_SKIPPED(seq)) res_publish(rs, seq, lo2 + lane, sm[oPUB + lane]);
            // (between the publish and the wait: the stacked restriction row s at the thread's two columns)
            const double s0 = tid < N2 ? sm[oP3C + tid] : 0.0, s1 = tid + BT < N2 ? sm[oP3C + tid + BT] : 0.0;
            double hv[2] = {0.0, 0.0};
            if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
            for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
            if (res_sweep<2>(rs, seq, N2, dead, D.tmo, hv, D.pollsleep)) {
                *fail = 1;
                if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (dbg) {
                const long long t_ = __builtin_amdgcn_s_memtime();
                dbg_acc[0] += t_;
                dbg_acc[4] -= t_;
            }
            const double v0 = tid < N2 ? hv[0] : 0.0, v1 = tid + BT < N2 ? hv[1] : 0.0;
            res_cs_rows(B2, v0, v1, sm + oPART, w, lane);
            const double ps = wave_sum(s0 * v0 + s1 * v1);
            const double p1 = nsp ? wave_sum(v0 + v1) : 0.0;
            if (lane == 0) {
                red[w] = ps;
                red[RES_WAVES + w] = p1;
            }
            if (dbg) {
                const long long t_ = __builtin_amdgcn_s_memtime();
                dbg_acc[4] += t_;
                dbg_acc[3] -= t_;
            }
            __syncthreads();
            if (dbg) dbg_acc[3] += __builtin_amdgcn_s_memtime();
            cls_end(RES_CL_RESTRICT);
            cls_begin(RES_CL_LEVEL2);
            ++seq;
            if (*fail) dead = true;   // (a give-up of r_2's sweep: the barrier has ordered the flag)
            if (w == 0 && lane < RES_WAVES) {
                const double wB = sm[oOWN + 6 * RES_WAVES + lane], mp = sm[oOWN + 7 * RES_WAVES + lane];
                const double T = res_red8_tree(sm + oPART + RES_WAVES * lane);
                const double sr = res_red8_tree(red), sum1 = res_red8_tree(red + RES_WAVES);
                const double d = res_pcg_1x1(sr + p2ws * sum1, h33, D.pcg_maxit);
                const double val = T + wB * sum1 + mp * d;
                if (pub && !RES_SKIPPED(seq)) res_publish(rs, seq, lo2 + lane, val);
            }
            // FULL: beta .* e_2, the prolongation's masked-sum operand, is formed at e_2's receipt by the thread that
            // receives the entry (oU is free: its last reader, the prolongation of the cycle before, lies hand-offs back)
            double be[2] = {0.0, 0.0};
            (void)be;
            if constexpr (FULL) {
                be[0] = sm[oBETA + tid];
                be[1] = sm[oBETA + tid + BT];
            }
            if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
            for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
            if (res_sweep<2>(rs, seq, N2, dead, D.tmo, hv, D.pollsleep)) {
                *fail = 1;
                if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (dbg) {
                const long long t_ = __builtin_amdgcn_s_memtime();
                dbg_acc[0] += t_;
                dbg_acc[4] -= t_;
            }
            if (tid < N2) sm[oE2 + tid] = hv[0];
            if (tid + BT < N2) sm[oE2 + tid + BT] = hv[1];
            if constexpr (FULL) {
                sm[oU + tid] = be[0] * hv[0];
                sm[oU + tid + BT] = be[1] * hv[1];
            }
            if (dbg) {
                const long long t_ = __builtin_amdgcn_s_memtime();
                dbg_acc[4] += t_;
                dbg_acc[5] -= t_;
            }
            __syncthreads();
            if (dbg) dbg_acc[5] += __builtin_amdgcn_s_memtime();
            cls_end(RES_CL_LEVEL2);
        }
    };

    // MG_Vcycle / MG_Wcycle from level 1 down; the correction ends in E1
    auto cycle = [&]() __attribute__((always_inline)) {
        const int nu = D.nu;
        // FULL: top() has left the C rows' totals of its local first half in PART, behind its barrier: the pre run's
        // first hand-off is published from them here, like a fed half sweep's
        if constexpr (FULL) cs_finish(false, false, false, seq + 1);
        for (int s = 0; s < nu; ++s) sweep1(false, s == 0, s == nu - 1, s == 0);
        if constexpr (FULL) {
            // rr = r - A e: the pre run's last half sweep has published the F block and left the workgroup's own
            // entries of the C block in RR1 (half1_cs).  The F block is all the restriction reads beside those: half
            // the granules, no row work and no publish barrier here.  It arrives pre-scaled by rho as below.
            ++seq;
            if (*fail) dead = true;   // (a give-up of that half sweep: its barrier has ordered the flag)
            const double rh0 = sm[oRHO + tid], rh1 = sm[oRHO + tid + BT];
            double hv[2] = {0.0, 0.0};
            if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
            for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
            if (res_sweep<2>(rs, seq, nf, dead, D.tmo, hv, D.pollsleep)) {
                *fail = 1;
                if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (dbg) {
                const long long t_ = __builtin_amdgcn_s_memtime();
                dbg_acc[0] += t_;
                dbg_acc[4] -= t_;
            }
            sm[oRR1 + tid] = hv[0] * rh0;
            sm[oRR1 + tid + BT] = hv[1] * rh1;
            if (dbg) {
                const long long t_ = __builtin_amdgcn_s_memtime();
                dbg_acc[4] += t_;
                dbg_acc[5] -= t_;
            }
            __syncthreads();
            if (dbg) dbg_acc[5] += __builtin_amdgcn_s_memtime();
        } else
        {   // rr = r - A e on both blocks
            if constexpr (CS1) {
                cls_begin(RES_CL_RR);
                cs_both_rows(oE1);
            } else {
            const double sF = wave_sum(res_rowdot_fma<KR1, 8 * oE1>(cF, aF, smb)) + dgF * sm[oE1 + rF];
            const double sC = wave_sum(res_rowdot_fma<KR1, 8 * oE1>(cC, aC, smb)) + dgC * sm[oE1 + rC];
            if (lane == 0) {
                sm[oPUB + w] = sm[oR1 + rF] - sF;
                sm[oPUB + RES_WAVES + w] = sm[oR1 + rC] - sC;
            }
            }
            if constexpr (CS1) {
                if (xm) {   // the F part arrives pre-scaled by rho for the mask-form restriction below
                    RES_HANDOFF_PV(4, N1, loF, hiF - loF, loC, hiC - loC, cs_row_value(oE1, false),
                                   { pa_[u_] = j < nf ? sm[oRHO + j] : 1.0; },
                                   { sm[oRR1 + j] = j < nf ? v * pa_[u_] : v; }, {}, 0, dum0, dum1);
                } else {
                    RES_HANDOFF_PV(4, N1, loF, hiF - loF, loC, hiC - loC, cs_row_value(oE1, false), {},
                                   { sm[oRR1 + j] = v; }, {}, 0, dum0, dum1);
                }
            } else
            if (xm) {   // the F part arrives pre-scaled by rho for the mask-form restriction below
                RES_HANDOFF_P(4, N1, loF, hiF - loF, loC, hiC - loC, { pa_[u_] = j < nf ? sm[oRHO + j] : 1.0; },
                              { sm[oRR1 + j] = j < nf ? v * pa_[u_] : v; }, {}, 0, dum0, dum1);
            } else {
                RES_HANDOFF(4, N1, loF, hiF - loF, loC, hiC - loC, { sm[oRR1 + j] = v; }, {}, 0, dum0, dum1);
            }
        }
        {   // r_2 = P' rr ; E2 := 0 ; c for the zero start
            cls_end(RES_CL_RR);
            cls_begin(RES_CL_RESTRICT);
            if (dbg) dbg_acc[6] -= __builtin_amdgcn_s_memtime();
            // row r2 of P' is [W(:,r2)' , 1 at nf + r2]; rowC == nf + row2 (level 2 = the C nodes)
            const double s = xm ? sm[oBETA + r2] * masked_sum(xbits >> 16, oRR1, nf) + sm[oRR1 + rC]
                                : res_csr_rowdot(D.Pt2, rowp[12 * w + 0], rowp[12 * w + 1], lane, sm, oRR1) +
                                      (RES_WIDENT ? sm[oRR1 + rC] : 0.0);
            if (dbg) dbg_acc[6] += __builtin_amdgcn_s_memtime();
            if (lane == 0) sm[oPUB + w] = s;
            if constexpr (POLY2) {   // ... and the whole visit of level 2 behind the one barrier of its receipt
                poly2_fed();
            } else {
            double sumr = 0.0;
            RES_HANDOFF(4, N2, lo2, hi2 - lo2, 0, 0, { sm[oR2 + j] = v; sm[oE2 + j] = 0.0; p0 += v; }, {},
                        (nsp ? 1 : 0), sumr, dum1);
            c2s = nsp ? sumr * rxx2 : 0.0;
            sumr2p = sumr;
            if (lfirst2 && !POLY2) {   // sweep2(true) of the first visit, same thread-to-entry map and sums
                const double cc = c2s;
                double p0 = 0.0;
                for (int j = tid; j < N2; j += BT) {
                    const double g_i = sm[oR2 + j] - sm[oAX2 + j] * cc;
                    const double en = sm[oDV2 + j] * g_i + cc;
                    sm[oE2 + j] = en;
                    p0 += sm[oR2 + j] - sm[oAX2 + j] * en;
                }
                if (nsp) {
                    p0 = wave_sum(p0);
                    if (lane == 0) red[w] = p0;
                }
                __syncthreads();
                if (nsp) c2s = res_red8(red) / xx2;
                __syncthreads();   // red is rewritten by the next hand-off
            }
            cls_end(RES_CL_RESTRICT);
            }
        }
        if constexpr (!POLY2)
            for (int leg = 0; leg < (D.wcycle ? 2 : 1); ++leg) visit2(leg == 1);      // MG_Wcycle.m:28-30
        {   // e_1 += P e_2                                                        MG_Vcycle.m:31
            cls_begin(RES_CL_PROLONG);
            if (dbg) dbg_acc[6] -= __builtin_amdgcn_s_memtime();
            // F rows: W(rowF,:) against E2 (A's columns nf + i are level-2 indices i); C rows: identity
            if constexpr (FULL) {
                // beta .* e_2 lies in oU since e_2's receipt (poly2_fed).  With P = [W; I] a C row's new value is
                // E1[nf + j] + E2[j]: thread j % BT, which holds both, adds them itself between the publish and the
                // wait, so the C block is not sent -- half the granules -- and its terms of the scalar are ready before
                // the wait.  They join the thread's sum behind the two F terms, the order of the four-granule form.
                const double sF = sm[oRHO + rF] * masked_sum(xbits & 0xffffu, oU, N2);
                if (dbg) dbg_acc[6] += __builtin_amdgcn_s_memtime();
                if (lane == 0) sm[oPUB + w] = sm[oE1 + rF] + sF;
                ++seq;
                if (*fail) dead = true;
                if (dbg) dbg_acc[3] -= __builtin_amdgcn_s_memtime();
                __syncthreads();
                if (dbg) dbg_acc[3] += __builtin_amdgcn_s_memtime();
                if (w == 0 && lane < RES_WAVES && !RES_SKIPPED(seq)) res_publish(rs, seq, loF + lane, sm[oPUB + lane]);
                double pa[2], pb[2], tc[2], hv[2] = {0.0, 0.0};
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int j = tid + u * BT;
                    pa[u] = sm[oR1 + j];
                    pb[u] = sm[oAX1 + j];
                    const double ec = sm[oE1 + nf + j] + sm[oE2 + j];
                    sm[oE1 + nf + j] = ec;
                    tc[u] = sm[oR1 + nf + j] - sm[oAX1 + nf + j] * ec;
                }
                if (dbg) dbg_acc[0] -= __builtin_amdgcn_s_memtime();
                for (int ps = 0; ps < D.presleep; ++ps) __builtin_amdgcn_s_sleep(1);
                if (res_sweep<2>(rs, seq, nf, dead, D.tmo, hv, D.pollsleep)) {
                    *fail = 1;
                    if (lane == 0) __hip_atomic_store(D.tmo, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (dbg) {
                    const long long t_ = __builtin_amdgcn_s_memtime();
                    dbg_acc[0] += t_;
                    dbg_acc[4] -= t_;
                }
                double p0 = 0.0;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    sm[oE1 + tid + u * BT] = hv[u];
                    p0 += pa[u] - pb[u] * hv[u];
                }
                p0 += tc[0];
                p0 += tc[1];
                // the F block as it arrives feeds the C rows of the first post-smoothing half sweep (see below)
                csBuf ^= 1;
                res_cs_rows(AC, hv[0], hv[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
                p0 = wave_sum(p0);
                if (lane == 0) red[w] = p0;
                if (dbg) {
                    const long long t_ = __builtin_amdgcn_s_memtime();
                    dbg_acc[4] += t_;
                    dbg_acc[5] -= t_;
                }
                __syncthreads();
                if (dbg) dbg_acc[5] += __builtin_amdgcn_s_memtime();
                c1 = res_red8_tree(red) * rxx1;
                eFo = sm[oE1 + loF + (lane & (RES_WAVES - 1))];
                eCo = sm[oE1 + loC + (lane & (RES_WAVES - 1))];
                cs_finish(false, true, false, seq + 1);
                csFed = 1;
                cls_end(RES_CL_PROLONG);
            } else {
            if (xm) {   // beta .* e_2 once per workgroup, then one masked sum per F row
                for (int j = tid; j < N2; j += BT) sm[oU + j] = sm[oBETA + j] * sm[oE2 + j];
                __syncthreads();
            }
            const double sF = xm ? sm[oRHO + rF] * masked_sum(xbits & 0xffffu, oU, N2)
                                 : res_csr_rowdot(D.P2, rowp[12 * w + 2], rowp[12 * w + 3], lane, sm, oE2);
            const double sC = RES_WIDENT ? sm[oE2 + r2]
                                       : res_csr_rowdot(D.P2, rowp[12 * w + 4], rowp[12 * w + 5], lane, sm, oE2);
            if (dbg) dbg_acc[6] += __builtin_amdgcn_s_memtime();
            if (lane == 0) {
                sm[oPUB + w] = sm[oE1 + rF] + sF;
                sm[oPUB + RES_WAVES + w] = sm[oE1 + rC] + sC;
            }
            double xig = 0.0;
            if constexpr (CS1) {
                // The F block as it arrives (granules t and t + BT of the hand-off: nf <= 2 BT) feeds the C rows of
                // the first post-smoothing half sweep, as a half sweep's receipt feeds the next one: behind the
                // closing barrier the finishing lanes publish it, and the run starts without a barrier of its own.
                const bool fedpost = FULL ? true : nu >= 1 && nf <= 2 * BT;
                double fe[2] = {0.0, 0.0};
                RES_HANDOFF_PVA(4, N1, loF, hiF - loF, loC, hiC - loC, sm[oPUB + lane],
                                { pa_[u_] = sm[oR1 + j]; pb_[u_] = sm[oAX1 + j]; },
                                {
                                    sm[oE1 + j] = v;
                                    p0 += pa_[u_] - pb_[u_] * v;
                                    if (u_ < 2 && j < nf) fe[u_] = v;
                                },
                                {
                                    if (fedpost) {
                                        csBuf ^= 1;
                                        res_cs_rows(AC, fe[0], fe[1], sm + oPART + RES_WAVES * RES_WAVES * csBuf, w, lane);
                                    }
                                },
                                {}, (nsp ? 1 : 0), xig, dum1);
                c1 = nsp ? xig * rxx1 : 0.0;
                if (fedpost) {
                    eFo = sm[oE1 + RES_OWN_ROW(loF, hiF, lane)];
                    eCo = sm[oE1 + RES_OWN_ROW(loC, hiC, lane)];
                    cs_finish(false, true, false, seq + 1);
                    csFed = 1;
                }
                cls_end(RES_CL_PROLONG);
            } else {
            RES_HANDOFF_P(4, N1, loF, hiF - loF, loC, hiC - loC, { pa_[u_] = sm[oR1 + j]; pb_[u_] = sm[oAX1 + j]; },
                          { sm[oE1 + j] = v; p0 += pa_[u_] - pb_[u_] * v; }, {}, (nsp ? 1 : 0), xig, dum1);
            c1 = nsp ? xig * rxx1 : 0.0;
            }
            }
        }
        // (column slices: the post run's first half sweep is fed by the prolongation, see above)
        for (int s = 0; s < nu; ++s) sweep1(true, false, s == nu - 1, s == 0 && csFed != 1);
    };

    auto add_correction = [&]() __attribute__((always_inline)) {   // x += e                                       Class_AMG.m:98,101
        if constexpr (FULL) {
            if (topfed) return;   // (added entry by entry in the post run's last half sweep: half1_cs)
        }
        for (int j = tid; j < N1; j += BT) sm[oX + j] = sm[oX + j] + sm[oE1 + j];
        __syncthreads();
    };

    // ---- Class_AMG.m:86-109 (one call site of every step: the kernel is large) -----------------
    const int maxit = D.maxit;
    const bool writer = b == 0 && tid == 0;
    const ResSolve sol = res_stationary(top, cycle, add_correction, D.retol, maxit, D.anycycle, fixed_cycles, dead, writer, out);
    if (RES_REMOTE && b == 0 && tid == 0)   // release the tail workgroup
        __hip_atomic_store(D.tail.tctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b == 0)
        for (int j = tid; j < N1; j += BT) xg[j] = sm[oX + j];
    if (writer) {
        out[0] = (double)sol.it;
        out[1] = sol.rel_res;
        out[2] = sol.res0;
        // any workgroup's give-up, not only this one's: a workgroup that gave up keeps publishing
        // (tagged, but computed from values it never received), so the iterate is void even when
        // workgroup 0 itself saw every hand-off arrive
        const unsigned anytmo = __hip_atomic_load(D.tmo, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        out[3] = (dead || anytmo != 0) ? 1.0 : 0.0;
        // column slices: a workgroup met an entry the layout has no slot for (an F row in an F column, a C row in a C
        // column) -- no time-out: the host drops the resident plan of this hierarchy and runs it as launches
        if (CS1 && __hip_atomic_load(D.tmo + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) out[3] = 2.0;
        // the last slot of the rhok block is never written by the iteration (it <= maxit): hand-offs of this
        // launch, chip-wide ones and visits of the remote tail (ipd_amg_resident_kernel)
        out[4 + 2 * (maxit + 2) - 1] = (double)(seq + tseq);
    }
    if (dbg) {
        D.dbg[0] = dbg_acc[0];
        D.dbg[1] = __builtin_amdgcn_s_memtime() - dbg_acc[1];
        D.dbg[2] = seq;
        D.dbg[3] = __builtin_amdgcn_s_memrealtime() - dbg_acc[2];
        D.dbg[4] = dbg_acc[3];
        D.dbg[5] = dbg_acc[4];
        D.dbg[6] = dbg_acc[5];
        D.dbg[7] = dbg_acc[6];
        D.dbg[8] = dbg_acc[7];
        if (CS1 && !RES_REMOTE) D.dbg[9] = dbg_acc[8];   // (a remote tail reports its busy time there)
        if constexpr (CS1)
            for (int k = 0; k < 2 * RES_NCLASS; ++k) D.dbg[16 + k] = (long long)cls_acc[k];
    }
#undef RES_REMOTE
#undef RES_WIDENT
#undef RES_OWN_ROW
#undef RES_SKIPPED
#undef RES_HANDOFF3
#undef RES_HANDOFF3R
#undef RES_HANDOFF4
#undef RES_HANDOFF
#undef RES_HANDOFF_P
#undef RES_HANDOFF_PV
#undef RES_HANDOFF_PVA
#undef dgF
#undef dvF
#undef bF
#undef dgC
#undef dvC
#undef bC
#undef dg2
#undef dv2
#undef dg3
#undef dv3
}
