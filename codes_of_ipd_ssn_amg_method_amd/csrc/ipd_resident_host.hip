// Host side of the resident kernels: the table of their instantiations, the execution of a plan
// (ipd_resident_plan.h decides, this file does the device work the plan calls for, verifies what only the device
// can verify and commits it to CycleState::res), the slots and the launch, the attach functions and the
// introspection entry points.  Its own kernels are the two checks; what it needs of the launch path's and the
// image unit's kernels it gets through their host functions (ipd_cycle_state.h).
#include "ipd_cycle_state.h"

#include <chrono>
#include <condition_variable>
#include <mutex>

#include "ipd_resident_big.h"   // (and ipd_resident.h: the descriptors and the kernel templates; ipd_resident_k*.hip instantiate them)

// The plan and what running it needs (opaque outside this unit: ipd_cycle_state.h)
struct ResidentState {
    bool ok = false;             // a plan is active
    bool off = false;            // IPD_NO_RESIDENT=1 when the hierarchy was set up
    ResidentPlan plan;
    ResDesc desc{};              // k_resident's descriptor (kept under a mask-form plan that replaced it: its rho)
    ResBigDesc big{};            // the mask-form kernel's
    unsigned skip_publish = 0;   // test hook (IPD_RES_DEBUG_SKIP_PUBLISH): fires on ONE launch
    unsigned char* block = nullptr;   // granule block, zeroed before every launch
    size_t block_bytes = 0;
    double* out = nullptr;
    int timeouts = 0;            // launches whose bounded spins gave up (then: multi-launch path)
    long long last_handoffs = 0;   // hand-offs and cycles of the last launch (ipd_amg_resident_kernel)
    int last_cycles = 0;
    bool last_full = false, last_diag = false;   // the variant the last launch took (ipd_amg_resident_variant)
    int capacity = -1;   // workgroups of the chosen instantiation the device holds at once (-1: not asked yet)
    int line_ke = 0, line_ke3 = 0;   // what the "[ipd] resident launch:" line shows as ke / ke3
    bool mask_form() const { return plan.kind == RESIDENT_BIG || plan.kind == RESIDENT_DEEP; }
};

// ---- the instantiations ---------------------------------------------------------------------
// Four units instantiate the kernels; this one takes their addresses and compiles none of them.
// ipd_resident_kbig.hip
extern template __global__ void k_resident_big<4, 2, true>(const ResBigDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident_big<8, 2, true>(const ResBigDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident_big<16, 1, false>(const ResBigDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident_big<32, 1, false>(const ResBigDesc, const double* __restrict__, double*, double*, int);
// ipd_resident_k2.hip
extern template __global__ void k_resident<16, 16, 0, true>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<4, 4, 0, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<8, 8, 0, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<16, 16, 0, false>(const ResDesc, const double* __restrict__, double*, double*, int);
// ipd_resident_kprod.hip
extern template __global__ void k_resident<16, 16, 0, true, false, true>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<16, 16, 0, true, true, true>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<16, 16, 0, true, false, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<16, 16, 0, false, false, false>(const ResDesc, const double* __restrict__, double*, double*, int);
// ipd_resident_k3.hip
extern template __global__ void k_resident<4, 4, 1, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<8, 8, 1, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<4, 4, 4, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<4, 4, 8, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<8, 8, 4, false>(const ResDesc, const double* __restrict__, double*, double*, int);
extern template __global__ void k_resident<8, 8, 8, false>(const ResDesc, const double* __restrict__, double*, double*, int);
// One row per instantiation: its name as a rocprofv3 kernel trace (and ipd_amg_resident_kernel) spells it, the
// plan's key, the kernel.  A key without a row is never launched -- the hierarchy takes the launches.
struct ResidentKernel {
    const char* name;
    ResidentKey key;
    const void* fn;
};
#define IPD_KFN(...) reinterpret_cast<const void*>(&__VA_ARGS__)
static const ResidentKernel RESIDENT_KERNELS[] = {
    {"k_resident_big<4,2,true>", ResidentKey::mask(4, 2, true), IPD_KFN(k_resident_big<4, 2, true>)},
    {"k_resident_big<8,2,true>", ResidentKey::mask(8, 2, true), IPD_KFN(k_resident_big<8, 2, true>)},
    {"k_resident_big<16,1,false>", ResidentKey::mask(16, 1, false), IPD_KFN(k_resident_big<16, 1, false>)},
    {"k_resident_big<32,1,false>", ResidentKey::mask(32, 1, false), IPD_KFN(k_resident_big<32, 1, false>)},
    {"k_resident<16,16,0,true>", ResidentKey::k(16, 0, true), IPD_KFN(k_resident<16, 16, 0, true>)},
    {"k_resident<4,4,0>", ResidentKey::k(4, 0, false), IPD_KFN(k_resident<4, 4, 0, false>)},
    {"k_resident<8,8,0>", ResidentKey::k(8, 0, false), IPD_KFN(k_resident<8, 8, 0, false>)},
    {"k_resident<16,16,0>", ResidentKey::k(16, 0, false), IPD_KFN(k_resident<16, 16, 0, false>)},
    {"k_resident<4,4,1>", ResidentKey::k(4, 1, false), IPD_KFN(k_resident<4, 4, 1, false>)},
    {"k_resident<8,8,1>", ResidentKey::k(8, 1, false), IPD_KFN(k_resident<8, 8, 1, false>)},
    {"k_resident<4,4,4>", ResidentKey::k(4, 4, false), IPD_KFN(k_resident<4, 4, 4, false>)},
    {"k_resident<4,4,8>", ResidentKey::k(4, 8, false), IPD_KFN(k_resident<4, 4, 8, false>)},
    {"k_resident<8,8,4>", ResidentKey::k(8, 4, false), IPD_KFN(k_resident<8, 8, 4, false>)},
    {"k_resident<8,8,8>", ResidentKey::k(8, 8, false), IPD_KFN(k_resident<8, 8, 8, false>)},
};
// The variants of those rows (ipd_resident_kprod.hip; k_resident's DIAG and FULL): the production forms of the
// column-slice kernels, without stamps and test hook, which every launch without a diagnostic request takes, and the
// full-shape forms of the composed instantiation.  A row of RESIDENT_KERNELS is the diagnostic general form of its
// key (for the kernels without a production form: the only one), and a variant reports that row's name.
struct ResidentVariant {
    ResidentKey key;   // (with `full`)
    bool diag;
    const void* fn;
};
static ResidentKey full_key(ResidentKey k) {
    k.full = true;
    return k;
}
static const ResidentVariant RESIDENT_VARIANTS[] = {
    {full_key(ResidentKey::k(16, 0, true)), false, IPD_KFN(k_resident<16, 16, 0, true, false, true>)},
    {full_key(ResidentKey::k(16, 0, true)), true, IPD_KFN(k_resident<16, 16, 0, true, true, true>)},
    {ResidentKey::k(16, 0, true), false, IPD_KFN(k_resident<16, 16, 0, true, false, false>)},
    {ResidentKey::k(16, 0, false), false, IPD_KFN(k_resident<16, 16, 0, false, false, false>)},
};
#undef IPD_KFN
// the row that names a key's instantiations (whatever the variant)
static const ResidentKernel* resident_kernel(ResidentKey key) {
    key.full = false;
    for (const ResidentKernel& k : RESIDENT_KERNELS)
        if (k.key == key) return &k;
    return nullptr;
}
// the kernel a launch of `key` takes, with or without diagnostics; *diag: what the kernel taken has
static const void* resident_kernel_fn(const ResidentKey& key, bool* diag) {
    for (const ResidentVariant& v : RESIDENT_VARIANTS)
        if (v.key == key && v.diag == *diag) return v.fn;
    if (key.full) return nullptr;   // (every full-shape key has both rows)
    const ResidentKernel* k = resident_kernel(key);
    *diag = true;
    return k ? k->fn : nullptr;
}

// ---- the checks a plan's execution launches ---------------------------------------------------
// *bad != 0 unless the level 1 <-> 2 transfers have the bigraph form P = [W; I] (AMG/transfer.m:19-25)
// entry for entry: every row of P' (level-2 row c) ends with the identity entry (column nf + c, value
// 1) and row nf + c of P is that identity entry alone.  The kernel then adds the identity parts
// itself: a 1025-entry row of P' is two 512-entry trips instead of three, and the C rows of P cost
// no trip at all.
__global__ void k_res_check_ident(int nf, int N2, ResCsr P, ResCsr Pt, int* __restrict__ bad) {
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < N2; c += gridDim.x * blockDim.x) {
        const int e1 = Pt.rp[c + 1], p0 = P.rp[nf + c];
        const bool ok = e1 > Pt.rp[c] && Pt.ci[e1 - 1] == nf + c && Pt.va[e1 - 1] == 1.0 &&
                        P.rp[nf + c + 1] - p0 == 1 && P.ci[p0] == c && P.va[p0] == 1.0;
        if (!ok) atomicOr(bad, 1);
    }
}

// rho of the mask-form transfers and the check of P against W(j,i) = s_ij beta_i rho_j (one wave per F row
// j: its row of P holds exactly the row's mask entries, in column order, each within 1e-12 of the form)
__global__ __launch_bounds__(256) void k_res_xmask_rho(int nf, int nc, int isnsp,
                                                       const unsigned long long* __restrict__ fbits, int nwf,
                                                       const double* __restrict__ alpha,
                                                       const double* __restrict__ beta,
                                                       const double* __restrict__ diag, const int* __restrict__ prp,
                                                       const int* __restrict__ pci, const double* __restrict__ pva,
                                                       double* __restrict__ rho, int* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int j = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= nf) return;
    double sb = 0.0;
    int cnt = 0;
    for (int w = 0; w < nwf; ++w) {
        const unsigned long long bits = fbits[(size_t)j * nwf + w];
        const int i = w * 64 + lane;
        if ((bits >> lane) & 1ull) sb += beta[i];
        cnt += __popcll(bits);
    }
    sb = wave_sum(sb);
    const double r = isnsp ? 1.0 / sb : alpha[j] / diag[j];
    if (lane == 0) rho[j] = r;
    bool wrong = (prp[j + 1] - prp[j]) != cnt;
    for (int t = prp[j] + lane; t < prp[j + 1] && !wrong; t += 64) {
        const int i = pci[t];
        const bool bit = i >= 0 && i < nc && ((fbits[(size_t)j * nwf + (i >> 6)] >> (i & 63)) & 1ull);
        const double ref = beta[i < nc ? i : 0] * r;
        if (!bit || !(fabs(pva[t] - ref) <= 1e-12 * fabs(ref))) wrong = true;
    }
    if (wrong) atomicExch(bad, 1);
}

// ---- the pieces a plan's execution is made of -------------------------------------------------
static ResidentInputs resident_inputs(const ipd_amg* h, const CycleState* st, const std::vector<LevelShape>& shapes) {
    ResidentInputs in;
    in.L = shapes.data();
    in.J = h->J;
    for (int k = 1; k <= std::min(3, h->J); ++k) in.S[k] = st->run[(size_t)k].dev.S;
    in.cycle = h->opts.cycle;
    in.smoth = h->opts.smoth;
    in.twogrid = h->opts.twogrid;
    in.bigph = h->opts.bigph;
    in.num_cu = st->num_cu;
    in.small_ok = st->small_ok;
    in.k_sub = st->k_sub;
    for (ImageRole r : {IMG_SUB, IMG_SUB3, IMG_SUB4})
        in.img[r] = ResidentImage{st->img[r].desc != nullptr, st->img[r].lds, st->img[r].bm};
    in.sub5 = st->sub5;
    return in;
}
static const SolveDesc* resident_image(const CycleState* st, ImageRole r) {
    return r == IMG_SUB || r == IMG_SUB3 || r == IMG_SUB4 ? st->img[r].desc : nullptr;
}

// level k's rows as the plan wants them: the launches' padded copy or a private one with stride p.S[k]
static LevelDev resident_rows(ipd_amg* h, const CycleState* st, const ResidentPlan& p, int k) {
    LevelDev d = st->run[(size_t)k].dev;
    if (!p.priv[k]) return d;
    d.S = p.S[k];
    build_padded_private(h, h->L[k].A, d.S, &d);
    return d;
}

// W(j,i) = s_ij beta_i rho_j: rho from the row sums (isnsp: rows normalised to sum 1, transfer.m:22-24)
// or alpha_j / A_jj, then every entry of P checked against the form; nullptr where P is not of it
static double* mask_transfer_rho(ipd_amg* h, const MaskOp& mo, int* bad) {
    ipd_ctx* ctx = h->ctx;
    double* rho = h->arena->alloc<double>((size_t)mo.nf);
    IPD_HIP(hipMemsetAsync(bad, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_res_xmask_rho, dim3(cdiv(mo.nf, 4)), dim3(256), 0, ctx->stream, mo.nf, mo.nc, h->opts.isnsp,
                       (const unsigned long long*)mo.fbits, mo.nwf, mo.alpha, mo.beta, mo.diag, h->L[2].P.rp,
                       h->L[2].P.ci, h->L[2].P.va, rho, bad);
    IPD_KERNEL_CHECK();
    return ctx->fetch1(bad) == 0 ? rho : nullptr;
}

static ResCsr res_csr(const Csr& m) { return ResCsr{m.rp, m.ci, m.va}; }
static ResLevelDesc res_level(const LevelDev& d) {
    return ResLevelDesc{d.N, d.nf, d.S, d.pci, d.pva, d.diag, d.dinv, d.Axi, d.xx};
}

template <class Desc>
static void set_cycle_options(Desc& D, const ipd_amg* h, int presleep) {
    D.nu = h->opts.smoth;
    D.isnsp = h->opts.isnsp;
    D.wcycle = h->opts.cycle == 'w';
    D.anycycle = (h->opts.cycle == 'w' || h->opts.cycle == 'v');
    D.maxit = h->opts.maxit;
    D.retol = h->opts.retol;
    D.pcg_maxit = h->opts.pcg_maxit;
    D.pollsleep = 1;   // (0..2 sleeps between polls made no difference, from 3 on it was worse)
    D.presleep = presleep;
    D.dbg_skip_seq = 0;
}

// The granule block, zeroed before every launch: [hand-off granules | time-out word] and, with a tail
// workgroup, [tin | tout: 2 x RES_GRAN_MAX granules each, by visit parity | tctl].  Fills the wire of T and the
// descriptor's time-out word and returns the granules.
static unsigned char* alloc_resident_block(ipd_amg* h, ResidentState& R, ResTail& T, unsigned*& tmo, size_t gran_bytes,
                                           bool tail) {
    const size_t tbytes = (size_t)RES_GRAN_MAX * 16;
    R.block_bytes = gran_bytes + 16 + (tail ? 4 * tbytes + 16 : 0);
    R.block = reinterpret_cast<unsigned char*>(h->arena->alloc_bytes(R.block_bytes));
    tmo = T.tmo = reinterpret_cast<unsigned*>(R.block + gran_bytes);
    T.tin = tail ? R.block + gran_bytes + 16 : R.block;                // never touched without
    T.tout = tail ? R.block + gran_bytes + 16 + 2 * tbytes : R.block;  // a tail workgroup
    T.tctl = tail ? reinterpret_cast<unsigned*>(R.block + gran_bytes + 16 + 4 * tbytes) : T.tmo;
    return R.block;
}

// level k in polynomial form, row layout (pack_bpoly), for the resident workgroups: form 64
static BPolyPack pack_resident_poly(ipd_amg* h, CycleState* st, int k, int seg, int ld) {
    const BPolyPack pb = pack_bpoly(h->ctx, h, st, k, h->opts.isnsp, 0, true, seg, ld);
    record_rows_op(st, h, k, pb);
    st->level_forms.resize((size_t)h->J + 1, 0);
    st->level_forms[(size_t)k] |= 64;
    return pb;
}

// the plan is taken: from here on the solve phase is one launch of p.key's instantiation
static void commit_resident(ipd_amg* h, ResidentState& R, const ResidentPlan& p, const PlanSwitches& sw) {
    R.plan = p;
    R.capacity = -1;
    R.skip_publish = sw.res_skip_publish;
    if (!R.out) R.out = h->arena->alloc<double>(4 + 2 * ((size_t)std::max(h->opts.maxit, 0) + 2));
    R.ok = true;
}

// The full-shape form of the composed instantiation: decided again whenever an attach call has changed what the
// predicate looks at (the composed level 2, the mask-form transfers)
static void choose_full_shape(const ipd_amg* h, const CycleState* st, ResidentState& R, const PlanSwitches& sw) {
    if (!R.ok || R.plan.kind != RESIDENT_K) return;
    const std::vector<LevelShape> shapes = level_shapes(h, st);
    const ResDesc& D = R.desc;
    const ResidentFullFacts facts{D.xm != 0, D.wident, D.isnsp, D.localfirst != 0};
    const bool full = resident_takes_full(R.plan, resident_inputs(h, st, shapes), facts, sw);
    if (full != R.plan.key.full) {
        R.plan.key.full = full;
        R.capacity = -1;   // (another instantiation: asked again before its first launch)
    }
}

// ---- k_resident: planned at amg_prepare_levels (ipd_cycle_state.h) -----------------------------
void prepare_resident(ipd_amg* h, CycleState* st, const std::vector<LevelShape>& shapes, const PlanSwitches& sw) {
    st->res = std::make_shared<ResidentState>();
    ResidentState& R = *st->res;
    R.off = sw.no_resident;   // (remembered: the mask-form kernel is set up later, by amg_attach_maskop)
    const ResidentPlan p = plan_resident(resident_inputs(h, st, shapes), sw);
    if (p.considered && switch_on("IPD_DEBUG_LEVELS"))
        std::fprintf(stderr, "[ipd] resident plan: J=%d nf=%d nc=%d S1=%d S2=%d S3=%d N4=%d Nt=%d k_sub=%d sub_lds=%zu\n", h->J,
                     h->L[1].nf, h->L[1].A.nr - h->L[1].nf, p.S[1], p.S[2], st->run[3].dev.S,
                     h->J >= 4 ? h->L[4].A.nr : 0, h->L[3].A.nr, st->k_sub, st->img[IMG_SUB].lds);
    if (p.kind == RESIDENT_NONE) return;
    const Level& l1 = h->L[1];
    const Level& l2 = h->L[2];
    const Level& l3 = h->L[3];
    const int N2 = l2.A.nr, nf = l1.nf;
    ResDesc D{};
    D.L1 = res_level(resident_rows(h, st, p, 1));
    D.L2 = res_level(resident_rows(h, st, p, 2));
    D.Pt2 = res_csr(l2.Pt);
    D.P2 = res_csr(l2.P);
    D.Pt3 = res_csr(l3.Pt);
    D.P3 = res_csr(l3.P);
    D.A3 = res_csr(l3.A);
    D.Nt = p.Nin;
    D.three = p.three ? 1 : 0;
    D.A4 = res_csr(p.three ? h->L[4].A : l3.A);
    if (p.three) {
        if (p.poly3) {
            const BPolyPack pb = pack_resident_poly(h, st, 3, 512, RES_P3_LD);
            D.p3rows = pb.M;
            D.p3w = pb.W;
            if (p.poly4) {
                const BPolyPack pb4 = pack_resident_poly(h, st, 4, RES_P4_SEG, RES_P4_LD);
                D.p4rows = pb4.M;
                D.p4w = pb4.W;
                D.N5 = h->L[5].A.nr;
            }
        }
        D.L3 = res_level(resident_rows(h, st, p, 3));
        D.Pt4 = res_csr(h->L[4].Pt);
        D.P4 = res_csr(h->L[4].P);
    } else {
        D.L3 = D.L2;   // unused
        D.Pt4 = res_csr(l3.Pt);
        D.P4 = res_csr(l3.P);
    }
    // s_sleep(1) count between a publish and the first poll (a failing poll delays the publishes it waits for).
    // Round 2: 0 -> 0.0869, 8 -> 0.0796, 12..14 -> 0.0770, 16 -> 0.0784 ms per V cycle.  With the shorter
    // hand-off of round 5 the best value moved down: metric workload 8 -> 0.0446, 13 -> 0.0456 ms
    // (6 / 7 / 9: 0.0450 / 0.0460 / 0.0447), W cycle 0.0852 against 0.0876, the sweep form of level 2 even.
    set_cycle_options(D, h, sw.res_presleep >= 0 ? sw.res_presleep : 8);
    D.wident = p.wident > 0 ? 1 : 0;
    if (p.wident < 0) {   // P = [W; I] to be verified
        int* bad = zeroed<int>(h->ctx, 1);
        hipLaunchKernelGGL(k_res_check_ident, dim3(cdiv(N2, 256)), dim3(256), 0, h->ctx->stream, nf, N2,
                           res_csr(l2.P), res_csr(l2.Pt), bad);
        IPD_KERNEL_CHECK();
        D.wident = h->ctx->fetch1(bad) == 0 ? 1 : 0;
    }
    D.localfirst = 1;
    const size_t gbytes = (size_t)RES_GRAN_MAX * 16;
    D.gran0 = alloc_resident_block(h, R, D.tail, D.tmo, 2 * gbytes, p.remote);
    D.gran1 = D.gran0 + gbytes;
    D.remote = p.remote ? 1 : 0;
    // the tail workgroup: rooted at level 3 it answers with P3 e_3 for level 2's rows, at level 4 with P4 e_4 for
    // level 3's -- or, below a polynomial level, with its root's iterate alone
    ResTail& T = D.tail;
    T.sub = resident_image(st, p.tail_image);
    T.root = p.tail_root;
    T.nin = p.tail_root == 5 ? D.N5 : D.Nt;
    T.nout = p.tail_root == 3 ? D.L2.N : D.L3.N;
    T.answer_root = D.p3rows != nullptr;
    T.Pout = p.tail_root == 3 ? D.P3 : D.P4;
    T.wcycle = D.wcycle;
    T.tail_bm = p.tail_bm ? 1 : 0;
    R.desc = D;
    R.line_ke = p.key.ke;
    R.line_ke3 = p.key.ke3;
    commit_resident(h, R, p, sw);
}

// Resident kernels need all their workgroups on the chip at once (one per CU): as many of them may
// run side by side as their grids fit into the device's CUs -- two of 128 workgroups on an MI355X
// (AMG4POT's two concurrent solves, bench.py --batch 2) -- and a further one waits for a free slot
// (a solve lasts a millisecond or two; running it as launches beside two resident kernels slows all
// three: --batch 4 fell from 2 x 20 M to 17.6 M DoF*cycles/s) and takes the multi-launch path only
// if none frees up within 50 ms.  (The spins are bounded, so an over-commitment could only cost the
// launch, never hang.)
struct ResidentSlots {
    std::mutex mu;
    std::condition_variable cv;
    int used[64] = {0};
    bool acquire(int device, int workgroups, int cus, int wait_ms) {
        std::unique_lock<std::mutex> lock(mu);
        if (workgroups > cus) return false;
        const bool got = cv.wait_for(lock, std::chrono::milliseconds(wait_ms),
                                     [&] { return used[device & 63] + workgroups <= cus; });
        if (!got) return false;
        used[device & 63] += workgroups;
        return true;
    }
    void release(int device, int workgroups) {
        {
            std::lock_guard<std::mutex> lock(mu);
            used[device & 63] -= workgroups;
        }
        cv.notify_all();
    }
};
static ResidentSlots& resident_slots() {
    static ResidentSlots s;
    return s;
}
struct ResidentLease {
    int device, wgs;
    bool ok;
    ResidentLease(int d, int w, int cus, int wait_ms)
        : device(d), wgs(w), ok(resident_slots().acquire(d, w, cus, wait_ms)) {}
    ~ResidentLease() {
        if (ok) resident_slots().release(device, wgs);
    }
};

// (ipd_cycle_state.h)
bool run_resident(ipd_amg* h, CycleState* st, const double* b_dev, double* x, int fixed_cycles,
                  std::vector<double>* out_host, float* ms, long long* dbg_dev) {
    ipd_ctx* ctx = h->ctx;
    ResidentState& R = *st->res;
    const ResidentPlan& p = R.plan;
    const int grid = p.grid();
    if (ctx->res_penalty > 0) {   // an earlier launch of this context gave up: stay on the launches for a while
        --ctx->res_penalty;
        return false;
    }
    // A remote-tail launch is 129 workgroups at M = 2048: two of them do not fit side by side, and a
    // realistic solve is a few milliseconds of mostly serial sub-cycle work -- waiting for the other
    // solve (AMG4POT's two right-hand sides) would serialise them, so the loser runs as launches
    // beside it at once.  The dense three-level launches (128 workgroups, two fit) keep waiting.
    ResidentLease lease(ctx->device, grid, st->num_cu, p.remote ? 0 : 50);
    if (!lease.ok) return false;
    ResDesc D = R.desc;
    D.dbg = D.tail.dbg = dbg_dev;
    D.dbg_skip_seq = R.skip_publish;
    ResBigDesc B = R.big;
    B.dbg_skip_seq = R.skip_publish;
    // stamps asked for, or the skip-publish hook about to fire: the instantiation that has them
    bool diag = dbg_dev != nullptr || R.skip_publish != 0;
    if (switch_on("IPD_DEBUG_LEVELS"))
        std::fprintf(stderr, "[ipd] resident launch: grid %d ke %d ke3 %d xm %d wident %d three %d remote %d\n", grid,
                     R.line_ke, R.line_ke3, D.xm, D.wident, D.three, D.remote);
    R.skip_publish = 0;   // the test hook fires on ONE launch
    IPD_HIP(hipMemsetAsync(R.block, 0, R.block_bytes, ctx->stream));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ms) {
        for (hipEvent_t& ev : ctx->tev)
            if (!ev) IPD_HIP(hipEventCreate(&ev));
        e0 = ctx->tev[0];
        e1 = ctx->tev[1];
        IPD_HIP(hipEventRecord(e0, ctx->stream));
    }
    // The workgroups spin on one another, so ALL of them must be on the chip at once: the grid is
    // checked against what the device can hold of this instantiation (registers, LDS: one workgroup
    // per CU) before the first launch; an oversized grid takes the multi-launch path for good -- and so
    // does a key the table has no row for.
    // (the capacity asked once serves a key's diagnostic and production forms: the launch's LDS admits one workgroup
    // per CU whatever the registers)
    const void* kern = resident_kernel_fn(p.key, &diag);
    if (kern) {
        IPD_OPTIN_LDS(ctx, kern, RES_LDS_MAX);
        if (R.capacity < 0) {
            int nb = 0;
            IPD_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, BT, p.lds));
            R.capacity = nb * st->num_cu;
        }
    }
    if (!kern || grid > R.capacity) {
        R.ok = false;
        return false;
    }
    R.last_full = p.key.full;
    R.last_diag = diag;
    void* args[] = {p.key.big ? (void*)&B : (void*)&D, (void*)&b_dev, (void*)&x, (void*)&R.out, (void*)&fixed_cycles};
    IPD_HIP(hipLaunchKernel(kern, dim3(grid), dim3(BT), args, p.lds, ctx->stream));
    IPD_KERNEL_CHECK();
    if (ms) IPD_HIP(hipEventRecord(e1, ctx->stream));
    const size_t nout = 4 + 2 * ((size_t)std::max(h->opts.maxit, 0) + 2);
    std::vector<double> out(nout);
    ctx->fetch(R.out, out.data(), nout);   // waits for the kernel (through the host mailbox: no stream synchronisation)
    if (ms) {
        IPD_HIP(hipEventSynchronize(e1));
        IPD_HIP(hipEventElapsedTime(ms, e0, e1));
    }
    if (out[3] == 2.0) {   // the column-slice layout cannot hold this level 1 (an entry of Aff or Acc off the diagonal):
        R.ok = false;      // no time-out and no penalty for the context -- this hierarchy runs as launches from now on
        return false;
    }
    if (out[3] != 0.0) {   // a bounded spin gave up somewhere (any workgroup: the kernel reports the
        // time-out word, not only workgroup 0's own view): not every workgroup was resident
        ++R.timeouts;
        ++ctx->res_giveups;
        ctx->res_penalty = 32 << std::min(ctx->res_giveups - 1, 6);
        if (R.timeouts >= 2) R.ok = false;
        return false;
    }
    R.last_handoffs = (long long)out[nout - 1];
    R.last_cycles = fixed_cycles > 0 ? fixed_cycles : (int)out[0];
    if (out_host) *out_host = std::move(out);
    return true;
}

bool resident_active(const CycleState* st) { return st->res->ok; }

// the "resident=..." field of amg_prepare_levels' debug line
void print_resident_summary(std::FILE* f, const CycleState* st) {
    std::fprintf(f, "resident=%d(G=%d,KE=%d)", (int)st->res->ok, st->res->plan.G, st->res->plan.key.ke);
}

// ---- the mask-form kernel: planned by amg_attach_maskop -----------------------------------------
// what both of its modes put into ResBigDesc
static ResBigDesc big_desc(ipd_amg* h, const CycleState* st, const MaskOp& mo, const LevelDev& d2, const double* rho) {
    ResBigDesc B{};
    B.nf = mo.nf;
    B.nc = mo.nc;
    B.N2 = mo.nc;
    B.S2 = d2.S;
    B.pci2 = d2.pci;
    B.pva2 = d2.pva;
    B.diag2 = d2.diag;
    B.dinv2 = d2.dinv;
    B.Axi2 = d2.Axi;
    B.xx2 = d2.xx;
    B.diag1 = mo.diag;
    B.dinv1 = st->run[1].dev.dinv;
    B.Axi1 = st->run[1].dev.Axi;
    B.xx1 = st->run[1].dev.xx;
    B.fbits = mo.fbits;
    B.cbits = mo.cbits;
    B.nwf = mo.nwf;
    B.nwc = mo.nwc;
    B.alpha = mo.alpha;
    B.beta = mo.beta;
    B.rho = rho;
    B.P3 = res_csr(h->L[3].P);   // (unused in DEEP mode)
    B.A3 = res_csr(h->L[3].A);
    set_cycle_options(B, h, 13);
    return B;
}
static void commit_mask_form(ipd_amg* h, ResidentState& R, const ResidentPlan& p, const ResBigDesc& B,
                             const PlanSwitches& sw) {
    R.big = B;
    R.line_ke3 = p.kind == RESIDENT_DEEP ? 1 : 0;   // (the launch line's ke stays a replaced plan's)
    commit_resident(h, R, p, sw);
}

// Derives the bit-mask form of level 1 from its CSR arrays; keeps the CSR kernels (returns
// false) unless A_1 is exactly Hybrid_AMG's rescaled operator for these p, q, tk.
//
// When it pays (`policy` true: the solvers' own call): the mask sweep moves 13x fewer bytes but is
// the slower launch while the level is latency-bound -- regime D at m = n = 1024 (2.1 M entries):
// 5.7 us against 5.2 us for the padded CSR sweep -- and the faster one once the CSR sweep is
// bandwidth-bound -- m = n = 2048 (8.4 M entries): 8.3 us against 13.4 us.  The solvers therefore
// attach it from 4 M entries on; IPD_MASKOP=1 lowers that to 16 entries per row, IPD_NO_MASKOP=1
// switches it off.  An explicit ipd_amg_attach_mask_operator call is not subject to the policy.
//
// The resident kernels' share (ipd_resident_plan.h): k_resident takes its level 1 <-> 2 transfers from the
// mask, and the mask-form kernel is planned here, its three-level mode (which IPD_RESIDENT_BIG=1 lets
// replace a k_resident plan, reusing its rho) or, when no plan exists, its deep mode.
bool amg_attach_maskop(ipd_amg* h, const double* p_dev, const double* q_dev, int m, int n, double tk,
                       bool policy, bool transfers_only) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    if (!st) return false;
    ResidentState& R = *st->res;
    const Level& lv = h->L[1];
    const PlanSwitches sw = read_plan_switches();
    const std::vector<LevelShape> shapes = level_shapes(h, st);
    const ResidentInputs in = resident_inputs(h, st, shapes);
    const ResidentFacts facts{m, n, R.off, R.ok, R.mask_form(), R.desc.wident != 0};   // (as the call finds them)
    const bool for_resident = resident_wants_mask_transfers(in, facts);
    bool sweeps_too = !transfers_only;
    const bool deep_cand = resident_deep_candidate(in, sw, facts);
    if (transfers_only && !for_resident && !sw.resident_big && !deep_cand) return false;
    if (policy) {
        if (!sw.maskop && (double)lv.A.nnz < 4.0e6) {
            if (!for_resident && !deep_cand) return false;
            sweeps_too = false;   // below the size where the mask SWEEPS of the launch path pay
        }
    }
    if (h->J < 2 || lv.nf != n || lv.N != m + n || tk == 0.0) return false;
    // a row of the mask costs nw word walks whatever its population: with fewer than ~16 entries
    // per row the padded CSR sweep always beats it
    if ((double)lv.A.nnz < 16.0 * lv.N) {
        if (!deep_cand) return false;
        sweeps_too = false;
    }
    if (std::max(m, n) > 4096) return false;   // a row's mask words must fit one wave (64 words)
    int* bad = ctx->scratch->alloc<int>(1);
    MaskOp mo;
    if (!build_maskop(h, p_dev, q_dev, m, n, tk, bad, &mo)) return false;
    if (for_resident && resident_mask_transfers_fit(in, facts)) {
        if (double* rho = mask_transfer_rho(h, mo, bad)) {
            ResDesc& D = R.desc;
            D.xm = 1;
            D.xm_nwf = mo.nwf;
            D.xm_nwc = mo.nwc;
            D.xm_fbits = mo.fbits;
            D.xm_cbits = mo.cbits;
            D.xm_beta = mo.beta;
            D.xm_rho = rho;
            choose_full_shape(h, st, R, sw);
        }
    }
    {
        const ResidentPlan p = plan_resident_big(in, sw, facts);
        if (p.kind == RESIDENT_BIG) {
            const LevelDev d2 = resident_rows(h, st, p, 2);
            const double* rho = R.desc.xm ? R.desc.xm_rho : mask_transfer_rho(h, mo, bad);
            if (rho) {
                ResBigDesc B = big_desc(h, st, mo, d2, rho);
                B.ranks = p.ranks;
                B.gran = alloc_resident_block(h, R, B.tail, B.tmo, (size_t)p.ranks * 2 * RB_GRAN * 16, false);
                commit_mask_form(h, R, p, B, sw);
            }
        }
    }
    if (deep_cand && !R.mask_form()) {
        const ResidentPlan p = plan_resident_deep(in, sw, facts);
        if (p.kind == RESIDENT_DEEP) {
            const LevelDev d2 = resident_rows(h, st, p, 2);
            if (const double* rho = mask_transfer_rho(h, mo, bad)) {
                const BPolyPack pb = pack_resident_poly(h, st, 3, RB_P3_SEG, RB_P3_LD);
                BPolyPack pb4;
                if (p.poly4) pb4 = pack_resident_poly(h, st, 4, RB_P4_SEG, RB_P4_LD);
                ResBigDesc B = big_desc(h, st, mo, d2, rho);
                B.N3 = h->L[3].A.nr;
                B.N4 = h->L[4].A.nr;
                B.Pt3 = res_csr(h->L[3].Pt);
                B.P3d = res_csr(h->L[3].P);
                B.p3rows = pb.M;
                B.p3w = pb.W;
                B.N5 = p.poly4 ? h->L[5].A.nr : 0;
                B.p4rows = pb4.M;
                B.p4w = pb4.W;
                B.gran = alloc_resident_block(h, R, B.tail, B.tmo, (size_t)2 * RB_GRAN * 16, true);
                // the tail workgroup answers with its root's iterate (level 3 or 4 applies M1 P itself)
                ResTail& T = B.tail;
                T.sub = resident_image(st, p.tail_image);
                T.root = p.tail_root;
                T.nin = p.poly4 ? B.N5 : B.N4;
                T.answer_root = 1;
                T.wcycle = B.wcycle;
                commit_mask_form(h, R, p, B, sw);
            }
        }
    }
    if (!sweeps_too) return R.desc.xm != 0 || R.mask_form();
    st->maskop = mo;
    st->mask_ok = true;
    // captured graphs (if any) were recorded with the CSR sweeps
    for (auto& g : st->gexec)
        if (g) {
            (void)hipGraphExecDestroy(g);
            g = nullptr;
        }
    return true;
}

// Level 2 of the level-resident kernel in polynomial form, composed over a whole visit (ResDesc::p2rows):
// three levels with a one-row tail, V cycle, 16-entry slices -- the metric's workload.  Packing costs five
// dense products of N2^3 (0.5 ms at N2 = 1024) against 18 us saved per cycle: it pays where many cycles run
// on one hierarchy (bench.py's fixed-hierarchy throughput), never in a solve of such a system, which takes one
// or two cycles -- so the solvers do not attach it themselves.
static bool amg_attach_poly2(ipd_amg* h) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    if (!st || !st->res->ok) return false;
    ResidentState& R = *st->res;
    if (!resident_takes_poly2(R.plan, resident_inputs(h, st, level_shapes(h, st)))) return false;
    const int seg = RES_NMAX / 2, ld = 2 * seg + 128;
    const BPolyPack pb = pack_bpoly(ctx, h, st, 2, h->opts.isnsp, 0, true, seg, ld);
    bpoly_compose(ctx, pb);
    R.desc.p2rows = pb.M;
    R.desc.p2w = pb.W;
    R.desc.p2seg = seg;
    R.desc.p2ld = ld;
    st->poly2_op = rows_op(pb);
    R.plan.key.poly2 = true;
    R.capacity = -1;   // (another instantiation: asked again before its first launch)
    choose_full_shape(h, st, R, read_plan_switches());
    st->level_forms.resize((size_t)h->J + 1, 0);
    st->level_forms[2] |= 128;
    ctx->sync();   // the pack's scratch operands die with the call scope
    return true;
}

extern "C" int ipd_amg_attach_level2_poly(ipd_amg* h, int32_t* attached) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        h->ctx->set_device();
        CallScope scope(h->ctx);
        const bool ok = amg_attach_poly2(h);
        if (attached) *attached = ok ? 1 : 0;
    });
}

static int attach_mask(ipd_amg* h, const double* p_dev, const double* q_dev, int64_t m, int64_t n, double tk,
                       int32_t* attached, bool transfers_only) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && p_dev && q_dev && m > 0 && n > 0, IPD_E_ARG, "bad argument");
        h->ctx->set_device();
        CallScope scope(h->ctx);
        const bool ok = amg_attach_maskop(h, p_dev, q_dev, (int)m, (int)n, tk, false, transfers_only);
        if (attached) *attached = ok ? 1 : 0;
    });
}
extern "C" int ipd_amg_attach_mask_operator(ipd_amg* h, const double* p_dev, const double* q_dev,
                                            int64_t m, int64_t n, double tk, int32_t* attached) {
    return attach_mask(h, p_dev, q_dev, m, n, tk, attached, false);
}
extern "C" int ipd_amg_attach_mask_transfers(ipd_amg* h, const double* p_dev, const double* q_dev,
                                             int64_t m, int64_t n, double tk, int32_t* attached) {
    return attach_mask(h, p_dev, q_dev, m, n, tk, attached, true);
}

// ---- introspection -----------------------------------------------------------------------------
// Mode 2 only: how many levels the resident workgroups keep in registers (2 or 3) and the level
// the tail is rooted at (3: the local tail of a three-level hierarchy or the remote tail workgroup's
// sub-cycle root; 4: remote tail below a resident level 3); zeros otherwise.
extern "C" int ipd_amg_resident_levels(const ipd_amg* h, int32_t* levels, int32_t* tail_root) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        const CycleState* st = h->cyc.get();
        const bool on = st && st->res->ok;
        if (levels) *levels = on ? st->res->plan.levels : 0;
        if (tail_root) *tail_root = on ? st->res->plan.tail_root : 0;
    });
}

// Which resident kernel this hierarchy's solve phase launches (mode 2 of ipd_amg_solve_mode) -- the
// instantiation's name as it appears in a rocprofv3 kernel trace, "" otherwise -- and what its last
// launch did: chip-wide hand-offs (tagged-granule exchanges, plus visits of the remote tail) and loop
// bodies.  bench.py derives hand-offs per cycle from these instead of re-deriving the kernel from sizes.
extern "C" int ipd_amg_resident_kernel(const ipd_amg* h, char* name, int32_t cap, int64_t* handoffs,
                                       int32_t* cycles, int32_t* mask_transfers) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && name && cap > 0, IPD_E_ARG, "bad argument");
        const CycleState* st = h->cyc.get();
        const ResidentKernel* kern = st && st->res->ok ? resident_kernel(st->res->plan.key) : nullptr;
        std::snprintf(name, (size_t)cap, "%s", kern ? kern->name : "");
        if (handoffs) *handoffs = st ? st->res->last_handoffs : 0;
        if (cycles) *cycles = st ? st->res->last_cycles : 0;
        // level 1 <-> 2 transfers from the bit mask: always in the mask-form kernel, ResDesc::xm otherwise
        if (mask_transfers) *mask_transfers = (st && st->res->ok && (st->res->mask_form() || st->res->desc.xm)) ? 1 : 0;
    });
}

// The variant of that kernel the hierarchy's last resident launch took: the full-shape form of the composed
// instantiation (resident_takes_full), and the form with stamps and test hook (a launch of ipd_amg_bench_resident /
// _classes, or one on which IPD_RES_DEBUG_SKIP_PUBLISH fired; kernels without a production form always have them).
// Zeros before the first launch.
extern "C" int ipd_amg_resident_variant(const ipd_amg* h, int32_t* full, int32_t* diag) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        const CycleState* st = h->cyc.get();
        if (full) *full = st && st->res->last_full ? 1 : 0;
        if (diag) *diag = st && st->res->last_diag ? 1 : 0;
    });
}

extern "C" int ipd_amg_solve_mode(const ipd_amg* h, int32_t* mode, int32_t* grid, int32_t* timeouts) {
    if (!h || !mode) return IPD_E_ARG;
    const CycleState* st = h->cyc.get();
    if (!st) return IPD_E_ARG;
    *mode = st->small_ok ? 1 : (st->res->ok ? 2 : 0);
    if (grid) *grid = st->res->ok ? st->res->plan.grid() : (st->small_ok ? 1 : 0);
    if (timeouts) *timeouts = st->res->timeouts;
    return IPD_OK;
}

// nst: words fetched (the column-slice kernels leave their stamps by class of hand-off in words 16 .. 31)
static int bench_resident_stamped(ipd_amg* h, const double* b_dev, double* x_dev, int cycles, double* total_ms,
                                  int64_t* stamps, int nst) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b_dev && x_dev && cycles > 0 && total_ms && stamps, IPD_E_ARG, "bad argument");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        CycleState* st = state_of(h);
        IPD_REQUIRE(st && st->res->ok, IPD_E_ARG, "hierarchy does not run in resident mode");
        const int N = h->L[1].A.nr;
        long long* dbg = ctx->scratch->alloc<long long>(32);
        IPD_HIP(hipMemsetAsync(dbg, 0, 256, ctx->stream));
        IPD_HIP(hipMemcpyAsync(h->x, x_dev, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice,
                               ctx->stream));
        float msf = 0.f;
        IPD_REQUIRE(run_resident(h, st, b_dev, h->x, cycles, nullptr, &msf, dbg), IPD_E_HIP,
                    "resident kernel gave up (not every workgroup was resident)");
        IPD_HIP(hipMemcpyAsync(x_dev, h->x, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice,
                               ctx->stream));
        long long hs[32];
        ctx->fetch(dbg, hs, (size_t)nst);
        for (int i = 0; i < nst; ++i) stamps[i] = hs[i];
        *total_ms = msf;
    });
}

extern "C" int ipd_amg_bench_resident(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                                      double* total_ms, int64_t stamps[10]) {
    return bench_resident_stamped(h, b_dev, x_dev, cycles, total_ms, stamps, 10);
}

extern "C" int ipd_amg_bench_resident_classes(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                                              double* total_ms, int64_t stamps[32]) {
    return bench_resident_stamped(h, b_dev, x_dev, cycles, total_ms, stamps, 32);
}
