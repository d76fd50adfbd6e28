// What the level-resident solve kernels share (device only; ipd_resident.h and ipd_resident_big.h include it): the hand-off protocol, the wire to the tail workgroup and that workgroup itself, the
// one-row tail's PCG and the stationary iteration with its stopping rules.
//
// Hand-off.  The only global traffic of a resident solve is the result of each step (a half sweep, a residual,
// a transfer): a row's new value is published as ONE 16-byte write-through (sc1) store of two self-tagged
// 8-byte granules {lo, tag, hi, tag} (MI355X guide, Guideline 16 R2: the data is the flag) and every workgroup
// sweeps all granules of the step with sc1 loads until every tag carries the step number.  Two buffers by step
// parity: a workgroup writes step t+2 only after it has seen all of step t+1, which every workgroup publishes
// only after it has read all of t (every workgroup owns at least one granule of every step -- a row, or an
// "ack" granule where it has none -- so "all of t+1" includes everyone).  tools/ubench_exchange.hip prices the
// step at 1.9 us (G = 128) against 4.6-5.0 us for the launch it replaces (profiles/r2_ubench_exchange.txt).
// The geometry of a buffer is the caller's: bytes per parity half, and -- rank groups, ResBigDesc::ranks -- the
// number of copies a publish writes and the byte base of the copy a sweep reads.
//
// Every spin is bounded: a workgroup that gives up raises the time-out word `tmo` (value = step number), every
// later sweep of every workgroup gives up at once, and the host falls back to the multi-launch path.
//
// Tail wire (ResTail).  Hierarchies deeper than the resident levels hand everything below them to ONE more
// workgroup, the last of the grid, which holds the LDS image of the single-workgroup sub-cycle (k_subcycle's
// code and data) and serves it: per visit the resident workgroups post the restricted residual of its root
// level into its inbox (tin, res_tail_post), it runs the V or W sub-cycle and publishes the answer (tout), and
// they wait for it with long sleeps (res_tail_answer).  Both boxes are 2 x RES_GRAN_MAX granules by visit
// parity; tctl[0] != 0 tells the tail workgroup that the solve is over.
#pragma once

#include "ipd_interp.h"

typedef unsigned int res_v4u __attribute__((ext_vector_type(4)));

static constexpr int RES_GRAN_MAX = RES_NMAX;  // granules per hand-off buffer (k_resident's, and the tail's boxes)
static constexpr unsigned RES_SPIN_MAX = 1u << 18;

struct ResCsr {
    const int* rp;
    const int* ci;
    const double* va;
};

// What the tail workgroup reads, and the wire the resident workgroups share with it; filled where a plan is
// executed (prepare_resident, the deep branch of amg_attach_maskop; alloc_resident_block for the wire).
// (The wire's pointers come first: the resident workgroups load them with the kernel arguments around them, and
// with the integers in front k_resident<4,4,4> / <4,4,8> spilled eleven more SGPRs, one more VGPR of spill lanes.)
struct ResTail {
    const SolveDesc* sub;   // LDS image of levels root..J (pack_image), NULL without a tail workgroup
    unsigned char* tin;     // inbox
    unsigned char* tout;    // outbox
    unsigned* tctl;         // [0] != 0: the solve is over, the tail workgroup leaves
    unsigned* tmo;          // [0] != 0: a bounded spin gave up (value = step number)
    long long* dbg;         // optional stamps (diagnostic build of the bench): see k_resident
    int root;               // the level the sub-cycle is rooted at (3, 4 or 5)
    int nin, nout;          // rows of the inbox (the root level) and of the outbox
    int answer_root;        // the answer is the root's iterate: the receivers prolongate it themselves (polynomial
                            // form of the level above); 0: Pout times it, nout rows of the level above
    ResCsr Pout;            // prolongation from the root level (unused with answer_root)
    int wcycle;             // both legs of MG_Wcycle.m:28-30 when the root is not the coarsest level
    int tail_bm;            // the launch's dynamic LDS has room for the image's operator copy (SolveDesc::bm_src)
};

// one fp64 value as two self-tagged 8-byte granules
__device__ __forceinline__ res_v4u res_pack(double v, unsigned tag) {
    res_v4u g;
    g.x = (unsigned)__double2loint(v);
    g.y = tag;
    g.z = (unsigned)__double2hiint(v);
    g.w = tag;
    return g;
}

// granule gidx of hand-off `seq`, into every rank group's copy of the buffer
__device__ __forceinline__ void res_publish(__amdgpu_buffer_rsrc_t rs, unsigned seq, int gidx, double v,
                                            int half_bytes = RES_GRAN_MAX * 16, int copies = 1) {
    for (int r = 0; r < copies; ++r)
        __builtin_amdgcn_raw_buffer_store_b128(res_pack(v, seq), rs,
                                               r * (2 * half_bytes) + (int)(seq & 1) * half_bytes + gidx * 16, 0,
                                               16 /* sc1: write-through */);
}

// One poll of the n granules at byte offset `base` (n <= NJ*BT); granule j goes to thread j % BT, pass
// u = j / BT.  Leaves the values in v[u]; true when every tag of the wave's granules carries `seq`.
template <int NJ>
__device__ __forceinline__ bool res_poll(__amdgpu_buffer_rsrc_t rs, int base, unsigned seq, int n, double (&v)[NJ]) {
    const int j0 = threadIdx.x;
    res_v4u gq[NJ];
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
        const int j = j0 + u * BT;
        gq[u] = __builtin_amdgcn_raw_buffer_load_b128(rs, base + (j < n ? j : 0) * 16, 0, 16 /* sc1 */);
    }
    bool ok = true;
#pragma unroll
    for (int u = 0; u < NJ; ++u) {
        const int j = j0 + u * BT;
        ok &= (j >= n) | ((gq[u].y == seq) & (gq[u].w == seq));
        v[u] = __hiloint2double((int)gq[u].z, (int)gq[u].x);
    }
    return __all(ok);
}

// Sweeps the n granules of hand-off `seq`: polls, a short sleep apart, until they have all arrived.  Returns
// true when the bounded spin gave up; the caller stores the values after the barrier it places (all waves
// have then finished the step's reads of the vectors that are about to change).
template <int NJ>
__device__ __forceinline__ bool res_sweep(__amdgpu_buffer_rsrc_t rs, unsigned seq, int n, bool dead,
                                          unsigned* tmo, double (&v)[NJ], int pollsleep = 1,
                                          int half_bytes = RES_GRAN_MAX * 16, int group_base = 0) {
    const int base = group_base + (int)(seq & 1) * half_bytes;
    unsigned spins = 0;
    bool bad = false;
    if (!dead) {
        for (;;) {
            if (res_poll<NJ>(rs, base, seq, n, v)) break;
            if (++spins > RES_SPIN_MAX ||
                ((spins & 255) == 255 &&
                 __hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                bad = true;
                break;
            }
            for (int ps = 0; ps < pollsleep; ++ps) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
        }
    }
    return bad;
}

// The wait of the slow hand-offs to and from the tail workgroup (tens of microseconds): long sleeps
// between polls, no give-up count -- it ends when every tag carries `seq` (returns 0), when the
// time-out word is raised (1) or when the exit word is (2; tail workgroup only, ctl may be NULL).
template <int NJ>
__device__ __forceinline__ int res_wait_slow(__amdgpu_buffer_rsrc_t rs, unsigned seq, int n,
                                             const unsigned* tmo, const unsigned* ctl, double (&v)[NJ]) {
    const int base = (int)(seq & 1) * (RES_GRAN_MAX * 16);
    for (unsigned spins = 0;; ++spins) {
        if (res_poll<NJ>(rs, base, seq, n, v)) return 0;
        if ((spins & 15) == 15) {
            if (__hip_atomic_load(tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return 1;
            if (ctl && __hip_atomic_load(ctl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return 2;
            if (spins > (1u << 21)) return 1;   // ~1 s: a sub-cycle leg takes 0.02-0.2 ms
        }
        __builtin_amdgcn_s_sleep(16);
        asm volatile("" ::: "memory");
    }
}

// ---- the tail wire, resident workgroups' side -------------------------------------------------------------
// row `row` of the restricted residual of visit `tseq` into the tail workgroup's inbox
__device__ __forceinline__ void res_tail_post(__amdgpu_buffer_rsrc_t rtin, unsigned tseq, int row, double v) {
    res_publish(rtin, tseq, row, v);
}

// Waits for the n values of the tail's answer to visit `tseq` (a dead workgroup does not wait).  A wait that
// ends without them raises the workgroup's `fail` flag and the time-out word (0x7fffffff: no step number).
// Returns res_wait_slow's status: hv holds the answer when it is 0 and the workgroup was not dead.
template <int NJ>
__device__ __forceinline__ int res_tail_wait(__amdgpu_buffer_rsrc_t rtout, unsigned tseq, int n, unsigned* tmo,
                                              int* fail, bool dead, int lane, double (&hv)[NJ]) {
    int st = 0;
    if (!dead) st = res_wait_slow<NJ>(rtout, tseq, n, tmo, nullptr, hv);
    if (st) {
        *fail = 1;
        if (lane == 0) __hip_atomic_store(tmo, 0x7fffffffu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return st;
}
// ... and leaves them at sm[off .. off + n) (zeros on failure) for the whole workgroup: one barrier, after which
// `dead` follows the flag.  tid / lane: the caller's copies of its indices (see RB_FRESH); sm and off apart, so that
// the address is formed as the kernels form theirs (index + constant).
template <int NJ>
__device__ __forceinline__ void res_tail_answer(__amdgpu_buffer_rsrc_t rtout, unsigned tseq, int n, unsigned* tmo,
                                                int* fail, bool& dead, double* sm, int off, int tid, int lane) {
    double hv[NJ];
    const int st = res_tail_wait<NJ>(rtout, tseq, n, tmo, fail, dead, lane, hv);
#pragma unroll
    for (int u = 0; u < NJ; ++u)
        if (tid + u * BT < n) sm[off + tid + u * BT] = (!dead && !st) ? hv[u] : 0.0;
    __syncthreads();
    if (*fail) dead = true;
}

// ---- the tail workgroup: k_subcycle's body as a server ------------------------------------------------------
// It loads the LDS image of levels root..J once, then for every visit waits for the restricted residual of its
// root level (T.nin <= BT granules in tin), runs the V or W sub-cycle rooted there out of LDS, and publishes
// the root's iterate or its prolongation to all rows of the level above (tout).  It leaves when the other
// workgroups raise the exit word (end of the solve) or the time-out word.
__device__ __forceinline__ void res_tail_workgroup(const ResTail& T, char* dyn_raw, PhaseLds* lds,
                                                   double* red, double* blkpart, int* stat) {
    const int tid = threadIdx.x, w = tid >> 6;
    SolveDesc* LD = sol_load_image(T.sub, dyn_raw);
    SolveCtx c = sol_ctx(LD, lds, red, blkpart, dyn_raw, nullptr);
    if (T.tail_bm && LD->bm_bytes) {   // one block-wide level's operator into LDS for the whole solve (SolveDesc::bm_src)
        const uint4* src = reinterpret_cast<const uint4*>(LD->bm_src);
        uint4* dst = reinterpret_cast<uint4*>(dyn_raw + LD->bm_off);
        for (int i = tid; i < LD->bm_bytes / 16; i += BT) dst[i] = src[i];
        __syncthreads();
        c.bm_lds = (unsigned)(size_t)(dyn_raw + LD->bm_off);
    }
    const int k0 = T.root, nin = T.nin, nout = T.nout;   // inbox / outbox rows
    const ResCsr& Pout = T.Pout;
    const bool two_legs = T.wcycle && k0 < LD->J;
    const auto rin = __builtin_amdgcn_make_buffer_rsrc(T.tin, 0, 2 * RES_GRAN_MAX * 16, 0x00020000);
    const auto rout = __builtin_amdgcn_make_buffer_rsrc(T.tout, 0, 2 * RES_GRAN_MAX * 16, 0x00020000);
    long long busy = 0;
    for (unsigned tseq = 1;; ++tseq) {
        double v[1];
        const int st = res_wait_slow<1>(rin, tseq, nin, T.tmo, T.tctl, v);
        if ((tid & 63) == 0) stat[w] = st;
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int k = 0; k < RES_WAVES; ++k) any |= stat[k];
        if (any) {                             // uniform: every wave reads the same eight words
            if (T.dbg && tid == 0) T.dbg[9] = busy;   // (diagnostic build of the bench: clocks between a request's arrival and its answer's stores)
            return;
        }
        const long long tb0 = (T.dbg && tid == 0) ? (long long)__builtin_amdgcn_s_memtime() : 0;
        if (tid < nin) LD->L[k0].lv.r[tid] = v[0];
        __syncthreads();
        sol_cycle(c, k0, false);
        __syncthreads();
        if (two_legs) {
            sol_cycle(c, k0, true);
            __syncthreads();
        }
        const double* e3 = sol_e(c, k0);
        if (T.answer_root) {
            if (tid < nin) res_publish(rout, tseq, tid, e3[tid]);
        } else
        for (int j = tid; j < nout; j += BT) {   // e += P e_root is finished by the receivers     MG_Vcycle.m:31
            double sd = 0.0;
            for (int t = Pout.rp[j]; t < Pout.rp[j + 1]; ++t) sd += Pout.va[t] * e3[Pout.ci[t]];
            res_publish(rout, tseq, j, sd);
        }
        if (T.dbg && tid == 0) busy += (long long)__builtin_amdgcn_s_memtime() - tb0;
        __syncthreads();                       // stat and e3 are rewritten by the next visit
    }
}

// PCG.m:68-87 (Jacobi-PCG, zero guess) on the 1 x 1 system h33 d = r, by every thread: the arithmetic of
// pcg_single.  Returns d.
__device__ __forceinline__ double res_pcg_1x1(double r, double h33, long long maxit) {
    double pp = r / h33, d = 0.0;
    double delta_new = r * pp;
    const double thresh = 1e-11 * 1e-11 * delta_new;
    for (long long it = 0; it < maxit && delta_new > thresh; ++it) {
        const double delta_old = delta_new;
        const double q = h33 * pp;
        const double alpha = delta_old / (q * pp);
        d += alpha * pp;
        r = r - alpha * q;
        const double wi = r / h33;
        delta_new = r * wi;
        pp = wi + (delta_new / delta_old) * pp;
    }
    return d;
}

// ---- Class_AMG.m:86-109: the stationary iteration and its stopping rules ----------------------------------
// top() forms r = b - A x and returns ||r||, cycle() leaves the correction of one V or W cycle and
// add_correction() adds it to x: the kernel's own steps, each with ONE call site here (the kernels are large).
// Every workgroup forms the same norm from the same values in the same order and so takes the same decision.
// `dead` is the kernel's give-up flag (its hand-offs set it).  The writer leaves rel_resk at out[4 ..] and rhok
// at out[4 + maxit + 2 ..] (the layout of k_solve_small).  fixed_cycles > 0: exactly that many loop bodies, no
// stopping rules (bench hook).
struct ResSolve {
    int it;
    double rel_res, res0;
};
template <class Top, class Cycle, class AddCorrection>
__device__ __forceinline__ ResSolve res_stationary(Top&& top, Cycle&& cycle, AddCorrection&& add_correction,
                                                   double retol, int maxit, int anycycle, int fixed_cycles,
                                                   const bool& dead, bool writer, double* out) {
    double* relk = out + 4;
    double* rhok = out + 4 + (maxit + 2);
    const bool fixed = fixed_cycles > 0;
    int it = 0, done = 0;
    double rel_res = 0.0, last_rel = 1.0, res = 0.0, res0 = 0.0, prev = 0.0;
    bool first = true;
    for (;;) {
        const double rnow = top();                                                // :89 / :103
        if (first) {
            first = false;
            res0 = res = rnow;
            if (!fixed) {
                if (res0 == 0.0) {                                                // :91-92
                    if (writer) {
                        relk[0] = 0.0;
                        rhok[0] = INFINITY;
                    }
                    break;
                }
                it = 1;                                                           // :94
                if (writer) {
                    relk[0] = 1.0;
                    rhok[0] = NAN;
                }
            }
        } else {
            prev = res;
            res = rnow;
            rel_res = res / res0;                                                 // :104
            const double rho = res / prev;                                        // :105
            if (fixed) {
                ++done;
            } else {
                if (writer) {
                    relk[it] = rel_res;
                    rhok[it] = rho;
                }
                last_rel = rel_res;
                ++it;
                if (rho > 1.0) break;                                             // :106
            }
        }
        if (dead) break;
        if (fixed ? done >= fixed_cycles : !(last_rel > retol && it <= maxit)) break;   // :95
        if (anycycle) {
            cycle();                                                              // :97-102
            add_correction();
        }
    }
    if (fixed)
        it = fixed_cycles;
    else if (res0 != 0.0)
        it -= 1;                                                                  // :108
    return ResSolve{it, rel_res, res0};
}
