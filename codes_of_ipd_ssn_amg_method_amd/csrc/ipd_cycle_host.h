// Host-side orchestration of the cycle (included by ipd_cycle.hip only): launch
// geometry, the recursive V/W schedule, the Class_AMG loop and the C ABI.  (The
// measurement hooks: ipd_cycle_bench.hip.)
#pragma once

#include "ipd_cycle_state.h"

__global__ void k_level_prepare(int N, int nf, const int* __restrict__ rp,
                                const int* __restrict__ ci, const double* __restrict__ va,
                                double* __restrict__ dinv, double* __restrict__ Axi,
                                int* __restrict__ maxoff) {
    // one wave per row: diagonal -> Rk, row sum -> A*1, longest off-diagonal row -> maxoff
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * blockDim.x) >> 6;
    int longest = 0;
    for (int r = wave; r < N; r += nwaves) {
        double s = 0.0, dg = 0.0;
        int hasd = 0;
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            s += va[t];
            if (ci[t] == r) {
                dg = va[t];
                hasd = 1;
            }
        }
        s = wave_sum(s);
        dg = wave_sum(dg);
        hasd = __any(hasd) ? 1 : 0;
        longest = max(longest, rp[r + 1] - rp[r] - hasd);
        if (lane == 0) {
            Axi[r] = s;
            // Class_AMG.m:56-59 (1./diag) for the bigraph GS, :72/:84 (0.5*(1./diag)) otherwise
            dinv[r] = nf > 0 ? 1.0 / dg : 0.5 * (1.0 / dg);
        }
    }
    // (thousands of waves on one address: 35 of the kernel's 41 us were this atomic; most waves find the
    // maximum already there)
    if (lane == 0 && longest > 0 && longest > __hip_atomic_load(maxoff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(maxoff, longest);
}

// All levels of a hierarchy in two launches instead of two per level (the hierarchy is rebuilt at every
// Newton step): workgroup b of k_levels_prepare belongs to the level whose block range holds b, workgroup
// k of k_levels_sum adds A*1 of level k in k_vec_sum's order (same bits).
constexpr int PREP_ML = 24;
struct PrepLevels {
    int n;
    int first_block[PREP_ML + 1];
    int N[PREP_ML], nf[PREP_ML];
    const int* rp[PREP_ML];
    const int* ci[PREP_ML];
    const double* va[PREP_ML];
    double* dinv[PREP_ML];
    double* Axi[PREP_ML];
    double* xx[PREP_ML];
    int* maxoff[PREP_ML];
};
__global__ void k_levels_prepare(const PrepLevels P) {
    int k = 0;
    while (k + 1 < P.n && (int)blockIdx.x >= P.first_block[k + 1]) ++k;
    const int nb = P.first_block[k + 1] - P.first_block[k], lb = blockIdx.x - P.first_block[k];
    const int N = P.N[k], nf = P.nf[k];
    const int* __restrict__ rp = P.rp[k];
    const int* __restrict__ ci = P.ci[k];
    const double* __restrict__ va = P.va[k];
    const int lane = threadIdx.x & 63;
    const int wave = (lb * blockDim.x + threadIdx.x) >> 6;
    const int nwaves = (nb * blockDim.x) >> 6;
    int longest = 0;
    for (int r = wave; r < N; r += nwaves) {
        double s = 0.0, dg = 0.0;
        int hasd = 0;
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            s += va[t];
            if (ci[t] == r) {
                dg = va[t];
                hasd = 1;
            }
        }
        s = wave_sum(s);
        dg = wave_sum(dg);
        hasd = __any(hasd) ? 1 : 0;
        longest = max(longest, rp[r + 1] - rp[r] - hasd);
        if (lane == 0) {
            P.Axi[k][r] = s;
            P.dinv[k][r] = nf > 0 ? 1.0 / dg : 0.5 * (1.0 / dg);
        }
    }
    // one atomic per workgroup (one per wave on one address cost 35 of the kernel's 41 us)
    __shared__ int bmax;
    if (threadIdx.x == 0) bmax = 0;
    __syncthreads();
    if (lane == 0 && longest > 0) atomicMax(&bmax, longest);
    __syncthreads();
    if (threadIdx.x == 0 && bmax > 0) atomicMax(P.maxoff[k], bmax);
}
__global__ __launch_bounds__(BT) void k_levels_sum(const PrepLevels P) {
    __shared__ double red[16];
    const int k = blockIdx.x;
    const double* v = P.Axi[k];
    double s = 0.0;
    for (int t = threadIdx.x; t < P.N[k]; t += BT) s += v[t];
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) P.xx[k][0] = tot;
}

// Builds the padded off-diagonal copy of width S (pad_width, ipd_launch_plan.h; 0: none)
static void pad_flush(ipd_ctx* ctx, PadBatch* b) {
    if (b->n == 0) return;
    int rows = 1;
    for (int q = 0; q < b->n; ++q) rows = std::max(rows, b->N[q]);
    hipLaunchKernelGGL(k_pad_build_batch, dim3(std::max(1, std::min(cdiv(rows, 4), 4096)), b->n), dim3(256), 0,
                       ctx->stream, *b);
    IPD_KERNEL_CHECK();
    b->n = 0;
}
static void build_padded(ipd_ctx* ctx, Arena& ar, const Csr& A, int S, LevelDev* dev, PadBatch* batch) {
    dev->pci = nullptr;
    dev->pva = nullptr;
    dev->diag = nullptr;
    if (S == 0) return;
    unsigned short* pci = ar.alloc<unsigned short>((size_t)A.nr * S);
    double* pva = ar.alloc<double>((size_t)A.nr * S);
    double* diag = ar.alloc<double>((size_t)A.nr);
    {   // (launched with the other levels' copies: pad_flush)
        if (batch->n == PAD_BATCH) pad_flush(ctx, batch);
        const int q = batch->n++;
        batch->N[q] = A.nr;
        batch->S[q] = S;
        batch->rp[q] = A.rp;
        batch->ci[q] = A.ci;
        batch->va[q] = A.va;
        batch->pci[q] = pci;
        batch->pva[q] = pva;
        batch->diag[q] = diag;
    }
    dev->pci = pci;
    dev->pva = pva;
    dev->diag = diag;
}

// Packs the polynomial form of level k (k_bpoly_*, ipd_cycle.hip) into the hierarchy's arena: LD-row
// column-major [Mr | Me | Mc] for the single-workgroup images, or (rows) the row-major layout the
// resident kernels' third level takes.
struct BPolyDev {
    double* M = nullptr;
    double* W = nullptr;
    int LD = 0;
    BPolyEntry e{};   // the pack's operands (scratch: valid until the call scope ends)
};
static BPolyDev pack_bpoly(ipd_ctx* ctx, ipd_amg* h, CycleState* st, int k, int isnsp, int LD, bool rows,
                           int rows_seg = 512, int rows_ld = RES_P3_LD) {
    Arena& ar = *h->arena;
    BPolyDev b;
    const Level& lv = h->L[k];
    const Csr& P = h->L[k + 1].P;
    const LevelDev& gd = st->run[(size_t)k].dev;
    const size_t N = (size_t)lv.A.nr, Nc = (size_t)P.nc, N8 = (N + 7) / 8 * 8, Nc8 = (Nc + 7) / 8 * 8;
    const size_t Np = (N + 15) / 16 * 16, Ncp = (Nc + 15) / 16 * 16, xcols = 2 * Np + 16;
    BPolyEntry e;
    e.Arp = lv.A.rp;
    e.Aci = lv.A.ci;
    e.Ava = lv.A.va;
    e.Prp = P.rp;
    e.Pci = P.ci;
    e.Pva = P.va;
    e.dinv = gd.dinv;
    e.Axi = gd.Axi;
    e.xx = gd.xx;
    e.N = (int)N;
    e.Nc = (int)Nc;
    e.Np = (int)Np;
    e.Ncp = (int)Ncp;
    e.nu = h->opts.smoth;
    e.isnsp = isnsp;
    e.LD = LD;
    // one zeroed block of scratch: A, S, P, T1, Pw[0], Pw[1], Y, dv, u, cs
    const size_t sc = 4 * Np * Np + 2 * Np * Ncp + Np * xcols + 3 * Np;
    double* blk = zeroed<double>(ctx, sc);
    e.A = blk;
    e.S = e.A + Np * Np;
    e.P = e.S + Np * Np;
    e.T1 = e.P + Np * Ncp;
    e.Pw[0] = e.T1 + Np * Ncp;
    e.Pw[1] = e.Pw[0] + Np * Np;
    e.Y = e.Pw[1] + Np * Np;
    e.dv = e.Y + Np * xcols;
    e.u = e.dv + Np;
    e.cs = e.u + Np;
    const size_t ncols = 2 * N8 + Nc8;
    const size_t out = rows ? (N + Nc) * (size_t)rows_ld + (N + Nc) : (size_t)LD * (ncols + 1);
    b.LD = LD;
    b.M = ar.alloc<double>(out);
    b.W = rows ? b.M + (N + Nc) * (size_t)rows_ld : b.M + (size_t)LD * ncols;
    IPD_HIP(hipMemsetAsync(b.M, 0, out * sizeof(double), ctx->stream));
    e.M = b.M;
    e.W = b.W;
    e.rows = rows ? b.M : nullptr;
    e.rows_seg = rows_seg;
    e.rows_ld = rows_ld;
    hipLaunchKernelGGL(k_bpoly_scatter, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, e);
    IPD_KERNEL_CHECK();
    hipLaunchKernelGGL(k_bpoly_colsum, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, e);
    IPD_KERNEL_CHECK();
    const int nS = (int)((N * N + 255) / 256), nT1 = (int)((Ncp / 16) * (Np / 16));   // one tile per workgroup
    hipLaunchKernelGGL(k_bpoly_S_T1, dim3((unsigned)(nS + nT1)), dim3(256), 0, ctx->stream, e, nS);
    IPD_KERNEL_CHECK();
    int cur = 0;
    const int nT = (int)((Np / 16) * (Np / 16));
    for (int s = 2; s <= e.nu; ++s) {
        const int nw = s == e.nu ? (int)((N + 3) / 4) : 0;
        hipLaunchKernelGGL(k_bpoly_step, dim3((unsigned)(nT + nw)), dim3(256), 0, ctx->stream, e, s, cur, nT);
        IPD_KERNEL_CHECK();
        cur ^= 1;
    }
    const int nZ = (int)((Ncp / 16) * (xcols / 16)), nC = (int)((Np / 16) * (Ncp / 16));
    const int nK = (int)((N * N + N + 255) / 256);
    hipLaunchKernelGGL(k_bpoly_final, dim3((unsigned)(nZ + nC + nK)), dim3(256), 0, ctx->stream, e, nZ, nC);
    IPD_KERNEL_CHECK();
    b.e = e;
    return b;
}

// what a row-layout pack holds (its own layout), for ipd_amg_packed_operator
static CycleState::RowsOp rows_op(const BPolyDev& b) {
    CycleState::RowsOp r;
    r.M = b.M;
    r.ld = b.e.rows_ld;
    r.seg = b.e.rows_seg;
    r.N = b.e.N;
    r.Nc = b.e.Nc;
    return r;
}
// one kernel's set of row-layout levels: level 3 is packed first and starts the set afresh, so that a
// hierarchy planned for one resident kernel and then for another never reports a mix of the two
static void record_rows_op(CycleState* st, const ipd_amg* h, int k, const BPolyDev& b) {
    if (k == 3) st->rows_ops.assign((size_t)h->J + 1, CycleState::RowsOp{});
    st->rows_ops.resize((size_t)h->J + 1);
    st->rows_ops[(size_t)k] = rows_op(b);
}

// The planners' switches, read at the call in which they take effect (amg_prepare_levels, amg_attach_maskop): the
// one place that reads them
static PlanSwitches read_plan_switches() {
    PlanSwitches s;
    s.no_pad = switch_on("IPD_NO_PAD");
    s.no_stage = switch_on("IPD_NO_STAGE");
    s.no_rrc = switch_on("IPD_NO_RRC");
    s.no_poly = switch_on("IPD_NO_POLY");
    s.no_blk = switch_on("IPD_NO_BLK");
    s.no_bpoly = switch_on("IPD_NO_BPOLY");
    s.no_blkdense = switch_on("IPD_NO_BLKDENSE");
    s.no_small = switch_on("IPD_NO_SMALL");
    s.no_subcycle = switch_on("IPD_NO_SUBCYCLE");
    s.no_resident = switch_on("IPD_NO_RESIDENT");
    s.no_resident_remote = switch_on("IPD_NO_RESIDENT_REMOTE");
    s.no_resident_three = switch_on("IPD_NO_RESIDENT_THREE");
    s.no_resident_deep = switch_on("IPD_NO_RESIDENT_DEEP");
    s.no_resident_big = switch_on("IPD_NO_RESIDENT_BIG");
    s.no_res_poly4 = switch_on("IPD_NO_RES_POLY4");
    s.resident_big = switch_on("IPD_RESIDENT_BIG");
    s.maskop = switch_on("IPD_MASKOP");
    if (const char* e = switch_value("IPD_RESIDENT_G")) s.resident_g = std::atoi(e);
    if (const char* e = switch_value("IPD_RESIDENT_RANKS")) s.resident_ranks = std::atoi(e);
    if (const char* e = switch_value("IPD_RES_PRESLEEP")) s.res_presleep = std::max(0, std::atoi(e));
    if (const char* e = switch_value("IPD_RES_DEBUG_SKIP_PUBLISH")) s.res_skip_publish = (unsigned)std::max(0, std::atoi(e));
    return s;
}

// the levels as the planners look at them
static std::vector<LevelShape> level_shapes(const ipd_amg* h, const CycleState* st) {
    std::vector<LevelShape> shapes((size_t)h->J + 1);
    for (int k = 1; k <= h->J; ++k) {
        const Level& lv = h->L[k];
        LevelShape& s = shapes[(size_t)k];
        s.nr = lv.A.nr;
        s.nnz = lv.A.nnz;
        s.nf = lv.nf;
        s.maxoff = st->run[(size_t)k].maxoff;
        s.p_nnz = k >= 2 ? lv.P.nnz : 0;
    }
    return shapes;
}

// the resident kernels: their table, the execution of a plan, the launch, the attach functions.  (Included
// here, ahead of the first launch of any other kernel template: the object lists its kernels in this order.)
#include "ipd_resident_host.h"

// Per-level vectors and constants (k_level_prepare), the launch plan of every level and the padded copies
// it asks for: st->run[k].plan, st->run[k].dev
static void prepare_level_runs(ipd_amg* h, CycleState* st, const LaunchSwitches& sw) {
    ipd_ctx* ctx = h->ctx;
    Arena& ar = *h->arena;
    // first pass: per-level vectors and the longest off-diagonal row of every level (one
    // readback for all levels), then the launch plan, second pass: padded copies and launch geometry
    int* maxoff = zeroed<int>(ctx, (size_t)h->J + 1);
    // levels whose constant data come from the donor hierarchy (see ipd_amg::donor)
    const ipd_amg* donor = h->donor.get();
    const CycleState* dst_ = donor ? donor->cyc.get() : nullptr;
    auto shared_level = [&](int k) { return dst_ && k <= 2 && k <= donor->J; };
    PrepLevels prep;
    prep.n = 0;
    prep.first_block[0] = 0;
    for (int k = 1; k <= h->J; ++k) {
        Level& lv = h->L[k];
        const int N = lv.A.nr;
        lv.N = N;
        lv.nf = (k == 1 && h->opts.bigph) ? (int)h->opts.fnode : 0;
        IPD_REQUIRE(lv.nf < N, IPD_E_ARG, "fnode must be smaller than the matrix size");
        const Level* dl = shared_level(k) ? &donor->L[k] : nullptr;
        lv.dinv = dl ? dl->dinv : ar.alloc<double>((size_t)N);
        lv.Axi = dl ? dl->Axi : ar.alloc<double>((size_t)N);
        lv.xx = dl ? dl->xx : ar.alloc<double>(1);
        lv.r = ar.alloc<double>((size_t)N);
        lv.e = ar.alloc<double>((size_t)N);
        lv.e2 = ar.alloc<double>((size_t)N);
        lv.w = ar.alloc<double>((size_t)N);
        lv.rr = ar.alloc<double>((size_t)N);
        if (dl) continue;
        if (prep.n < PREP_ML) {
            const int q = prep.n++;
            prep.N[q] = N;
            prep.nf[q] = lv.nf;
            prep.rp[q] = lv.A.rp;
            prep.ci[q] = lv.A.ci;
            prep.va[q] = lv.A.va;
            prep.dinv[q] = lv.dinv;
            prep.Axi[q] = lv.Axi;
            prep.xx[q] = lv.xx;
            prep.maxoff[q] = maxoff + k;
            prep.first_block[q + 1] = prep.first_block[q] + std::max(1, std::min(cdiv(N, 16), 4096));
        } else {
            hipLaunchKernelGGL(k_level_prepare, dim3(std::max(1, std::min(cdiv(N, 4), 4096))), dim3(256),
                               0, ctx->stream, N, lv.nf, lv.A.rp, lv.A.ci, lv.A.va, lv.dinv, lv.Axi,
                               maxoff + k);
            IPD_KERNEL_CHECK();
            hipLaunchKernelGGL(k_vec_sum, dim3(1), dim3(BT), 0, ctx->stream, (const double*)lv.Axi, N,
                               lv.xx);
            IPD_KERNEL_CHECK();
        }
    }
    if (prep.n > 0) {
        hipLaunchKernelGGL(k_levels_prepare, dim3(prep.first_block[prep.n]), dim3(256), 0, ctx->stream, prep);
        IPD_KERNEL_CHECK();
        hipLaunchKernelGGL(k_levels_sum, dim3(prep.n), dim3(BT), 0, ctx->stream, prep);
        IPD_KERNEL_CHECK();
    }
    std::vector<int> hmax((size_t)h->J + 1);
    ctx->fetch(maxoff, hmax.data(), (size_t)h->J + 1);
    std::vector<LaunchShape> shapes((size_t)h->J + 1);
    for (int k = 1; k <= h->J; ++k) {
        const Level& lv = h->L[k];
        LaunchShape& s = shapes[(size_t)k] = LaunchShape{lv.A.nr, lv.A.nnz, lv.nf, hmax[(size_t)k]};
        if (k == h->J) break;
        const Level& cl = h->L[k + 1];
        s.Pt = MatShape{cl.Pt.nr, cl.Pt.nc, cl.Pt.nnz};
        s.P = MatShape{cl.P.nr, cl.P.nc, cl.P.nnz};
        s.t1 = cl.T1.rp != nullptr;
        s.T1 = MatShape{cl.T1.nr, cl.T1.nc, cl.T1.nnz};
    }
    LaunchLevel dplan[3];   // the donor's records: its padded copy goes with its geometry
    int dlevels = 0;
    for (int k = 1; k <= 2 && shared_level(k); ++k) dplan[dlevels = k] = dst_->run[(size_t)k].plan;
    const std::vector<LaunchLevel> plan = plan_launches(shapes.data(), h->J, ctx->num_cu, sw, dplan, dlevels);
    PadBatch pads;   // the levels' padded copies: one launch after the loop
    for (int k = 1; k <= h->J; ++k) {
        Level& lv = h->L[k];
        LevelRun& rn = st->run[(size_t)k];
        rn.plan = plan[(size_t)k];
        rn.dev.N = lv.N;
        rn.dev.nf = lv.nf;
        rn.dev.S = rn.plan.S;
        rn.dev.L = rn.plan.L;
        rn.dev.G = rn.plan.G;
        rn.dev.rp = lv.A.rp;
        rn.dev.ci = lv.A.ci;
        rn.dev.va = lv.A.va;
        rn.dev.dinv = lv.dinv;
        rn.dev.Axi = lv.Axi;
        rn.dev.xx = lv.xx;
        rn.dev.r = lv.r;
        rn.dev.rr = lv.rr;
        if (shared_level(k)) {
            const LevelDev& dd = dst_->run[(size_t)k].dev;
            rn.dev.pci = dd.pci;
            rn.dev.pva = dd.pva;
            rn.dev.diag = dd.diag;
        } else {
            build_padded(ctx, ar, lv.A, rn.plan.S, &rn.dev, &pads);
            rn.maxoff = hmax[(size_t)k];
        }
    }
    pad_flush(ctx, &pads);
}

// Restriction / prolongation arguments of the launches, the coarsest level's PCG, the solve's vectors
static void prepare_transfers(ipd_amg* h, CycleState* st) {
    Arena& ar = *h->arena;
    auto xfer = [](const Csr& m, const XferPlan& xp, const double* x, double* y, int add) {
        // nrows, ncols, L, G, row0, row1, rp, ci, va, x, y, add, staged
        return XferArgs{m.nr, m.nc, xp.L, xp.G, 0, m.nr, m.rp, m.ci, m.va, x, y, add, xp.staged ? 1 : 0};
    };
    for (int k = 1; k < h->J; ++k) {
        Level& fine = h->L[k];
        Level& coarse = h->L[k + 1];
        LevelRun& rn = st->run[(size_t)k];
        // restriction: rows of P' (coarse rows), gathers the fine residual
        rn.restrict_args = xfer(coarse.Pt, rn.plan.rest, fine.rr, coarse.r, 0);
        // prolongation: rows of P (fine rows), gathers the coarse correction
        rn.prolong_args = xfer(coarse.P, rn.plan.prol, coarse.e, fine.e, 1);
    }
    {   // coarsest level: PCG(A,r) with the 2-argument defaults (PCG.m:18-23)
        Level& cl = h->L[h->J];
        PcgArgs a;
        a.N = cl.A.nr;
        a.L = st->run[(size_t)h->J].plan.pcg_L;
        a.rp = cl.A.rp;
        a.ci = cl.A.ci;
        a.va = cl.A.va;
        a.rhs = cl.r;
        a.guess = nullptr;
        a.d = cl.e;
        a.work = ar.alloc<double>(4 * (size_t)cl.A.nr);
        a.tol = 1e-11;
        a.maxit = h->opts.pcg_maxit;
        a.precd = 2;
        a.out = nullptr;
        a.nresk = 0;
        st->run[(size_t)h->J].pcg = a;
    }
    st->num_cu = h->ctx->num_cu;
    st->hist = ar.alloc<double>(8);
    st->x2 = ar.alloc<double>((size_t)h->L[1].A.nr);
    h->x = ar.alloc<double>((size_t)h->L[1].A.nr);
    h->b = ar.alloc<double>((size_t)h->L[1].A.nr);
}

// in one workgroup a row is walked by few lanes: re-picked without widening
static int lanes_in_one_workgroup(int nnz, int rows) {
    const double avg = (double)nnz / std::max(rows, 1);
    int L = 1;
    while (L < 64 && (double)L * 6.0 < avg) L <<= 1;
    return L;
}

// Descriptor of image `spec` before its layout: every level's global arrays and its lanes per row in one workgroup
static void fill_desc(ipd_amg* h, const CycleState* st, const ImageSpec& spec, SolveDesc* sd) {
    std::memset(sd, 0, sizeof(SolveDesc));
    sd->J = h->J;
    sd->nu = h->opts.smoth;
    sd->isnsp = h->opts.isnsp;
    sd->wcycle = h->opts.cycle == 'w';
    sd->anycycle = (h->opts.cycle == 'w' || h->opts.cycle == 'v');
    sd->maxit = h->opts.maxit;
    sd->retol = h->opts.retol;
    sd->pcg = st->run[(size_t)h->J].pcg;
    for (int k = 1; k <= h->J; ++k) {
        SolveLevel& sl = sd->L[k];
        sl.lv = st->run[(size_t)k].dev;
        sl.lv.S = 0;  // the single-workgroup kernels walk the CSR arrays only
        const Level& lv = h->L[k];
        sl.lv.L = lanes_in_one_workgroup(lv.A.nnz, lv.A.nr);
        sl.lv.G = 1;
        sl.e = lv.e;
        sl.e2 = lv.e2;
        sl.w = lv.w;
        sl.nnzA = lv.A.nnz;
        sl.nnzP = k < h->J ? h->L[k + 1].P.nnz : 0;
        if (k < h->J) {
            sl.rest = st->run[(size_t)k].restrict_args;
            sl.prol = st->run[(size_t)k].prolong_args;
            for (XferArgs* xa : {&sl.rest, &sl.prol}) {
                xa->L = lanes_in_one_workgroup(xa == &sl.rest ? h->L[k + 1].Pt.nnz : h->L[k + 1].P.nnz, xa->nrows);
                xa->G = 1;
                xa->staged = 1;
                xa->row0 = 0;
                xa->row1 = xa->nrows;
            }
        }
    }
    sd->k_lds = spec.k_lds;
    sd->k_semi = spec.k_semi;
    sd->k_tiny = spec.k_tiny;
    sd->k_blk = spec.k_blk;
    sd->stage_bytes = (int)spec.stage_bytes;
    if (spec.role != IMG_SOLVE) {
        sd->root_r = h->L[spec.k_lds].r;
        sd->root_e = h->L[spec.k_lds].e;
    }
}

// What packs an image on the device: the constant arrays copied into it, the dense / lane-map / polynomial
// blocks computed into it, and the relocations of the descriptor's LDS offsets
struct ImagePack {
    std::vector<PackEntry> packs;
    std::vector<unsigned> relocs;
    std::vector<DenseEntry> dense;
    std::vector<LmapEntry> lmaps;
    std::vector<PolyEntry> polys;
    size_t poly_lds = 0;   // dynamic LDS of k_pack_poly
};

// Packs the bound image on the device and records the levels' forms; with bm_extra, one block-wide
// polynomial operator's LDS copy goes behind the image's `off` bytes (*bm_extra: its size, 0 = none).
static SolveDesc* upload_image(ipd_ctx* ctx, ipd_amg* h, CycleState* st, SolveDesc* sd, int k_from, size_t off,
                               size_t image_bytes, ImagePack& lay, size_t* bm_extra) {
    Arena& ar = *h->arena;
    // One block-wide polynomial level's operator as an LDS copy (SolveDesc::bm_src), for the launches that can
    // afford bm_bytes more dynamic LDS (the resident kernels' tail workgroup): the deepest such level whose
    // stacked operator has at most 128 rows and fits behind the work vectors.
    sd->bm_src = nullptr;
    sd->bm_level = sd->bm_ld = sd->bm_off = sd->bm_bytes = 0;
    if (bm_extra) {
        *bm_extra = 0;
        for (int k = h->J - 1; k >= std::max(2, k_from); --k) {
            const SolveLevel& T = sd->L[k];
            if (!T.gM || T.gLD != 128) continue;
            const size_t N = (size_t)T.lv.N, Nc = (size_t)h->L[k + 1].A.nr, rows = N + Nc;
            if (rows > 128) continue;
            const size_t ld = (rows + 1) & ~size_t(1), ncols = 8 * (2 * ((N + 7) / 8) + (Nc + 7) / 8);
            const size_t need = 8 * ld * (ncols + 1);   // (ld even: a multiple of 16; the vector W behind the columns)
            if (off + need > IMAGE_LDS_OPTIN) continue;
            double* cp = ar.alloc<double>(ld * (ncols + 1));
            hipLaunchKernelGGL(k_bm_compact, dim3((unsigned)ncols + 1), dim3(128), 0, ctx->stream, T.gM, 128, cp,
                               (int)ld, T.gW, (int)rows);
            IPD_KERNEL_CHECK();
            sd->bm_src = cp;
            sd->bm_level = k;
            sd->bm_ld = (int)ld;
            sd->bm_off = (int)off;
            sd->bm_bytes = (int)need;
            *bm_extra = need;
            break;
        }
    }
    char* img = reinterpret_cast<char*>(ar.alloc_bytes(image_bytes));
    // the image head and the pack descriptors go up in ONE copy: [head | packs | dense | lmaps | polys] in
    // a scratch block, the head then moves into the image as one more entry of k_pack_image
    const size_t o_packs = plan_r16(SOL_HEAD), o_dense = o_packs + plan_r16((lay.packs.size() + 1) * sizeof(PackEntry)),
                 o_lmaps = o_dense + plan_r16(lay.dense.size() * sizeof(DenseEntry)),
                 o_polys = o_lmaps + plan_r16(lay.lmaps.size() * sizeof(LmapEntry)),
                 o_end = o_polys + plan_r16(lay.polys.size() * sizeof(PolyEntry));
    char* stg = reinterpret_cast<char*>(ctx->scratch->alloc_bytes(o_end));
    std::vector<char> hb(o_end, 0);
    std::memcpy(hb.data(), sd, sizeof(SolveDesc));
    std::memcpy(hb.data() + plan_r16(sizeof(SolveDesc)), lay.relocs.data(), lay.relocs.size() * sizeof(unsigned));
    {
        PackEntry he{};
        he.src = stg;
        he.dst_off = 0;
        he.bytes = (unsigned)SOL_HEAD;
        lay.packs.push_back(he);
    }
    std::memcpy(hb.data() + o_packs, lay.packs.data(), lay.packs.size() * sizeof(PackEntry));
    if (!lay.dense.empty()) std::memcpy(hb.data() + o_dense, lay.dense.data(), lay.dense.size() * sizeof(DenseEntry));
    if (!lay.lmaps.empty()) std::memcpy(hb.data() + o_lmaps, lay.lmaps.data(), lay.lmaps.size() * sizeof(LmapEntry));
    if (!lay.polys.empty()) std::memcpy(hb.data() + o_polys, lay.polys.data(), lay.polys.size() * sizeof(PolyEntry));
    ctx->upload_bytes(stg, hb.data(), o_end);
    hipLaunchKernelGGL(k_pack_image, dim3((unsigned)lay.packs.size()), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const PackEntry*>(stg + o_packs), img);
    IPD_KERNEL_CHECK();
    if (!lay.dense.empty()) {
        hipLaunchKernelGGL(k_pack_dense, dim3((unsigned)lay.dense.size()), dim3(256), 0, ctx->stream,
                           reinterpret_cast<const DenseEntry*>(stg + o_dense), img);
        IPD_KERNEL_CHECK();
    }
    if (!lay.lmaps.empty()) {
        hipLaunchKernelGGL(k_pack_lmap, dim3((unsigned)lay.lmaps.size()), dim3(BT), 0, ctx->stream,
                           reinterpret_cast<const LmapEntry*>(stg + o_lmaps), img);
        IPD_KERNEL_CHECK();
    }
    if (!lay.polys.empty()) {
        IPD_OPTIN_LDS(ctx, k_pack_poly, IMAGE_LDS_OPTIN);
        hipLaunchKernelGGL(k_pack_poly, dim3((unsigned)lay.polys.size()), dim3(BT), lay.poly_lds, ctx->stream,
                           reinterpret_cast<const PolyEntry*>(stg + o_polys), img);
        IPD_KERNEL_CHECK();
    }
    st->level_forms.resize((size_t)h->J + 1, 0);
    for (int k = std::max(k_from, sd->k_blk); k <= h->J; ++k) {
        const SolveLevel& T = sd->L[k];
        if (k == sd->k_semi) continue;
        st->level_forms[(size_t)k] |= T.gM ? 16 : T.pMr ? (k >= sd->k_tiny ? 8 : 32) : k >= sd->k_tiny ? 4 : T.blk_dense ? 2 : 1;
    }
    return reinterpret_cast<SolveDesc*>(img);
}

static const char* const IMAGE_ROLE_NAMES[] = {"solve", "sub", "sub3", "sub4", "none"};

// the descriptor's pointer that piece (level, slot) of a layout stands for: its place in SolveLevel, or in the
// SolveDesc itself for the image-wide slots
#define IPD_LV(m) offsetof(SolveLevel, m)
static const size_t SLOT_FIELD[SLOT_COUNT] = {
    IPD_LV(lv.rp), IPD_LV(lv.ci), IPD_LV(lv.va), IPD_LV(lv.dinv), IPD_LV(lv.Axi), IPD_LV(lv.xx),
    IPD_LV(rest.rp), IPD_LV(rest.ci), IPD_LV(rest.va), IPD_LV(prol.rp), IPD_LV(prol.ci), IPD_LV(prol.va),
    IPD_LV(lmap), IPD_LV(dA), IPD_LV(dP), IPD_LV(dPt), IPD_LV(pMr), IPD_LV(pMe), IPD_LV(pMc), IPD_LV(pW),
    IPD_LV(lv.r), IPD_LV(e), IPD_LV(e2), IPD_LV(lv.rr), IPD_LV(w),
    offsetof(SolveDesc, bp_part), offsetof(SolveDesc, pcg.work), IPD_LV(rest.x), IPD_LV(rest.y),
    offsetof(SolveDesc, pcg.rp), offsetof(SolveDesc, pcg.ci), offsetof(SolveDesc, pcg.va)};
#undef IPD_LV
static size_t* slot_field(SolveDesc* sd, int level, ImageSlot slot) {   // (every one is a pointer: read and written as its bits)
    const bool wide = slot == SLOT_BP_PART || slot == SLOT_PCG_WORK || slot >= SLOT_PCG_RP;
    return reinterpret_cast<size_t*>(reinterpret_cast<char*>(wide ? (void*)sd : (void*)&sd->L[level]) + SLOT_FIELD[slot]);
}

// Binds the layout to the descriptor: every piece's pointer becomes its LDS offset and one relocation, every
// copied or computed piece one pack entry
static ImagePack bind_layout(ipd_ctx* ctx, ipd_amg* h, CycleState* st, const std::vector<LevelShape>& shapes, const LevelPlan& plan,
                             const ImageSpec& spec, const ImageLayout& lay, SolveDesc* sd) {
    ImagePack pk;
    for (int k = spec.k_lds; k <= h->J; ++k) {
        const LevelPieces own = plan.pieces(shapes.data(), spec, k);
        if (own.form == FORM_SEMI) continue;   // matrix, transfers, dinv, Axi stay in global memory
        // a form that has no piece for one of the level's arrays does not read it
        for (int q = SLOT_RP; q <= SLOT_PROL_VA; ++q)
            if (!own.has((ImageSlot)q)) *slot_field(sd, k, (ImageSlot)q) = 0;
        sd->L[k].blk_dense = own.form == FORM_BDENSE;
        if (own.form != FORM_BPOLY) continue;
        st->poly_ops.resize((size_t)h->J + 1);   // the operators stay in global memory
        CycleState::PolyOp& po = st->poly_ops[(size_t)k];
        if (!po.M) {   // packed once for all images
            const BPolyDev b = pack_bpoly(ctx, h, st, k, sd->isnsp, (int)own.ld(), false);
            po = CycleState::PolyOp{b.M, b.W, b.LD, h->L[k].A.nr, h->L[k + 1].A.nr};
        }
        sd->L[k].gM = po.M;
        sd->L[k].gW = po.W;
        sd->L[k].gLD = po.LD;
    }
    for (const ImagePiece& p : lay.pieces) {
        size_t* field = slot_field(sd, p.level, p.slot);
        const void* src = reinterpret_cast<const void*>(*field);   // the global array, where the piece is a copy of one
        *field = p.off;
        pk.relocs.push_back((unsigned)(reinterpret_cast<char*>(field) - reinterpret_cast<char*>(sd)));
        const int k = p.level;
        const unsigned dst = (unsigned)(p.off - spec.stage_bytes);
        if (p.kind == PIECE_COPY) pk.packs.push_back(PackEntry{src, dst, (unsigned)p.bytes});
        if (p.kind == PIECE_LMAP) pk.lmaps.push_back(LmapEntry{h->L[k].A.rp, h->L[k].A.nr, dst});
        if (p.kind == PIECE_DENSE) {
            const Csr& m = p.slot == SLOT_DA ? h->L[k].A : p.slot == SLOT_DP ? h->L[k + 1].P : h->L[k + 1].Pt;
            pk.dense.push_back(DenseEntry{m.rp, m.ci, m.va, m.nr, m.nc, dst, sd->L[k].blk_dense ? bdense_ld(m.nr) : 0});
        }
        if (p.kind != PIECE_POLY) continue;
        if (p.slot == SLOT_PMR) {   // pMr, pMe, pMc, pW follow one another: one entry of k_pack_poly
            const Level& lv = h->L[k];
            const Csr& P = h->L[k + 1].P;
            const LevelDev& gd = st->run[(size_t)k].dev;   // global pointers (the descriptor's are LDS offsets by now)
            const size_t N = (size_t)lv.A.nr, Nc = (size_t)P.nc;
            sd->L[k].pLD = (int)plan.pieces(shapes.data(), spec, k).ld();
            pk.polys.push_back(PolyEntry{lv.A.rp, lv.A.ci, lv.A.va, P.rp, P.ci, P.va, gd.dinv, gd.Axi, gd.xx, (int)N, (int)Nc,
                                         sd->nu, sd->isnsp, sd->L[k].pLD, 0, 0, 0, 0});
            pk.poly_lds = std::max(pk.poly_lds, 8 * (5 * N * N + 2 * N * Nc + 4 * N) + 64);
        }
        PolyEntry& pe = pk.polys.back();
        (p.slot == SLOT_PMR ? pe.offMr : p.slot == SLOT_PME ? pe.offMe : p.slot == SLOT_PMC ? pe.offMc : pe.offW) = dst;
    }
    return pk;
}

// Packs image `spec` as image_layout lays it out (levels k_lds..J behind the staging area) and stores it in st
// by its role
static void pack_image(ipd_ctx* ctx, ipd_amg* h, CycleState* st, const std::vector<LevelShape>& shapes, const LevelPlan& plan,
                       const ImageSpec& spec) {
    std::unique_ptr<SolveDesc> sdp(new SolveDesc());
    SolveDesc* sd = sdp.get();
    fill_desc(h, st, spec, sd);
    CycleState::Image& out = st->img[spec.role];
    st->solve_cached = st->solve_cached || (spec.role == IMG_SOLVE && spec.k_lds <= h->J);
    if (spec.k_lds > h->J) {   // a solve with nothing in LDS: the descriptor as it is
        out.desc = reinterpret_cast<SolveDesc*>(h->arena->alloc_bytes(sizeof(SolveDesc)));
        out.lds = spec.lds;
        ctx->upload_bytes(out.desc, sd, sizeof(SolveDesc));
        return;
    }
    const ImageLayout lay = image_layout(shapes.data(), plan, spec);
    // what is packed is what the planner admitted (a rooted image's prediction may count levels above the root)
    IPD_REQUIRE(lay.total <= spec.lds && lay.total <= IMAGE_LDS_OPTIN, IPD_E_LIMIT, "LDS image: larger than planned");
    IPD_REQUIRE(lay.pieces.size() <= (size_t)RELOC_MAX, IPD_E_LIMIT, "LDS image: too many relocations");
    ImagePack pk = bind_layout(ctx, h, st, shapes, plan, spec, lay, sd);
    sd->image_bytes = (int)lay.image_bytes;
    const char* skip = switch_value("IPD_DEBUG_SKIP");
    sd->dbg_skip = skip ? std::atoi(skip) : 0;
    sd->lds_total = (int)lay.total;
    sd->nreloc = (int)pk.relocs.size();
    out.desc = upload_image(ctx, h, st, sd, spec.k_lds, lay.total, lay.image_bytes, pk, spec.role == IMG_SOLVE ? nullptr : &out.bm);
    out.lds = lay.total;
}

void amg_prepare_levels(ipd_amg* h) {
    std::unique_ptr<CycleState> st(new CycleState());
    st->run.resize((size_t)h->J + 1);
    const PlanSwitches sw = read_plan_switches();
    prepare_level_runs(h, st.get(), sw);
    prepare_transfers(h, st.get());
    // single-workgroup kernels: which levels, in which form, in which LDS images (ipd_level_plan.h)
    const std::vector<LevelShape> shapes = level_shapes(h, st.get());
    PlanOptions po;
    po.cycle = h->opts.cycle;
    po.smoth = h->opts.smoth;
    po.twogrid = h->opts.twogrid;
    po.concurrent_pair = h->opts.concurrent_pair;
    const LevelPlan plan = plan_levels(shapes.data(), h->J, po, sw);
    const bool debug = switch_on("IPD_DEBUG_LEVELS");
    if (debug)
        for (int k = 1; k <= h->J; ++k)
            std::fprintf(stderr, "[ipd] launch plan: %s\n", launch_plan_line(st->run[(size_t)k].plan, k, h->J).c_str());
    if (debug)
        for (const ImageSpec& s : plan.images)
            std::fprintf(stderr, "[ipd] image %s: k_lds=%d k_semi=%d k_tiny=%d k_blk=%d stage=%zu lds=%zu%s\n",
                         IMAGE_ROLE_NAMES[s.role], s.k_lds, s.k_semi, s.k_tiny, s.k_blk, s.stage_bytes, s.lds,
                         plan.sub5 == s.role ? " (level-5 tail)" : "");
    ipd_ctx* ctx = h->ctx;
    IPD_OPTIN_LDS(ctx, k_solve_small<true>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_solve_small<false>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_pcg_small<true>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_pcg_small<false>, IMAGE_LDS_OPTIN);
    IPD_OPTIN_LDS(ctx, k_subcycle, IMAGE_LDS_OPTIN);
    st->k_sub = plan.k_sub;
    st->sub_semi_root = plan.sub_semi_root;
    for (const ImageSpec& s : plan.images) pack_image(ctx, h, st.get(), shapes, plan, s);
    if (plan.small_ok) {
        st->solve_out = h->arena->alloc<double>(4 + 2 * ((size_t)std::max(h->opts.maxit, 0) + 2));
        st->small_ok = true;
    }
    st->sub5 = plan.sub5;
    prepare_resident(h, st.get(), shapes, sw);
    if (debug) {
        std::fprintf(stderr, "[ipd] J=%d small=%d k_sub=%d ", h->J, (int)st->small_ok, st->k_sub);
        print_resident_summary(stderr, st.get());
        std::fprintf(stderr, " levels:");
        for (int k = 1; k <= h->J; ++k) std::fprintf(stderr, " %d/%d", h->L[k].A.nr, h->L[k].A.nnz);
        std::fprintf(stderr, "\n");
    }
    h->cyc = std::shared_ptr<CycleState>(st.release());
}

// ---------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------
// ---- fused-program emitter (which phases are queued: phase_is_small, ipd_launch_plan.h) -------
void flush_fused(ipd_ctx* ctx, CycleState* st) {
    if (st->pending.n == 0) return;
    hipLaunchKernelGGL(k_fused, dim3(1), dim3(BT), st->pending_lds, ctx->stream, st->pending);
    IPD_KERNEL_CHECK();
    st->pending.n = 0;
    st->pending_lds = 0;
}

static PhaseDesc& push_phase(ipd_ctx* ctx, CycleState* st, int type, int stage_len) {
    if (st->pending.n == FUSED_MAX) flush_fused(ctx, st);
    PhaseDesc& d = st->pending.d[st->pending.n++];
    d.type = type;
    d.pad_ = 0;
    st->pending_lds = std::max(st->pending_lds, sizeof(double) * (size_t)stage_len);
    return d;
}

// Runs `launch(r0, r1, grid)` over the row range `rg` of a matrix walked by L lanes per row.  Unsharded: one
// call with the planned grid.  Sharded: this rank's slice only (its grid: the slice's own), followed by one
// grouped RCCL all-gather of the vectors the launch produced (each rank wrote its own slice of every one of them).
template <class F>
static void run_rows(ipd_ctx* ctx, CycleState* st, const RowRange& rg, int L, F launch,
                     std::initializer_list<double*> produced) {
    flush_fused(ctx, st);  // big launch: everything queued before it must run first
    const int G = st->shard_ranks;
    const int lo = rg.r0, rows = rg.r1 - rg.r0;
    if (G <= 1 || rows % G != 0 || rows < st->shard_min_rows) {  // replicated level
        launch(rg.r0, rg.r1, rg.G);
        return;
    }
    const int cnt = rows / G, grid = pick_blocks(cnt, L, st->num_cu);
    if (st->shard_emulate) {
        for (int vr = 0; vr < G; ++vr) launch(lo + vr * cnt, lo + (vr + 1) * cnt, grid);
        return;
    }
    launch(lo + st->shard_rank * cnt, lo + (st->shard_rank + 1) * cnt, grid);
    double* bases[4];
    int nv = 0;
    for (double* v : produced)
        if (v) bases[nv++] = v + lo;
    comm_allgather_inplace(ctx, bases, nv, cnt);
}

static void launch_smooth(ipd_ctx* ctx, const SmoothArgs& a, int grid) {
    const size_t dyn = a.staged ? sizeof(double) * (size_t)a.lv.N : 0;
    dispatch_staged_pad(a.staged, a.lv.S > 0, [&](auto S, auto P) {
        hipLaunchKernelGGL((k_smooth<decltype(S)::value, decltype(P)::value>), dim3(grid), dim3(BT), decltype(S)::value ? dyn : 0, ctx->stream, a);
    });
    IPD_KERNEL_CHECK();
}

// a restriction or prolongation as planned: queued into the fused program or launched over its rows
static void issue_xfer(ipd_ctx* ctx, CycleState* st, XferArgs a, const XferPlan& xp) {
    if (xp.queued) {
        push_phase(ctx, st, PH_XFER, a.ncols).u.x = a;
        return;
    }
    const size_t dyn = a.staged ? sizeof(double) * (size_t)a.ncols : 0;
    run_rows(ctx, st, RowRange{0, a.nrows, xp.G}, a.L,
             [&](int r0, int r1, int grid) {
                 a.row0 = r0;
                 a.row1 = r1;
                 if (a.staged)
                     hipLaunchKernelGGL(k_xfer<true>, dim3(grid), dim3(BT), dyn, ctx->stream, a);
                 else
                     hipLaunchKernelGGL(k_xfer<false>, dim3(grid), dim3(BT), 0, ctx->stream, a);
                 IPD_KERNEL_CHECK();
             },
             {a.y});
}

static void launch_resid(ipd_ctx* ctx, const LevelRun& rn, const double* e, int r0, int r1,
                         int grid) {
    const size_t dyn = rn.plan.staged ? sizeof(double) * (size_t)rn.dev.N : 0;
    dispatch_staged_pad(rn.plan.staged, rn.dev.S > 0, [&](auto S, auto P) {
        hipLaunchKernelGGL((k_resid<decltype(S)::value, decltype(P)::value>), dim3(grid), dim3(BT), decltype(S)::value ? dyn : 0, ctx->stream, rn.dev, e, r0, r1);
    });
    IPD_KERNEL_CHECK();
}

// one smoother sweep on level k: Jacobi = one launch, bigraph GS = two half launches
void launch_sweep(ipd_amg* h, CycleState* st, int k, int isnsp, bool post) {
    ipd_ctx* ctx = h->ctx;
    Level& lv = h->L[k];
    LevelRun& rn = st->run[(size_t)k];
    SmoothArgs a;
    a.lv = rn.dev;
    a.eold = lv.e;
    a.enew = lv.e2;
    a.win = lv.w;
    a.wout = lv.w;
    a.isnsp = isnsp;
    a.staged = rn.plan.staged;
    a.eold_zero = rn.e_zero ? 1 : 0;
    const LaunchLevel& p = rn.plan;
    // How a range is issued: queued into the fused program (replicated on every rank), or as launches of the
    // bit-mask kernel (level 1 with a mask operator: same two half sweeps, 1 bit per matrix entry; sharded runs
    // give each owner its block of the half's rows -- a row range inside one half is all the kernel needs) or
    // of the rows kernel
    const bool mask = k == 1 && lv.nf > 0 && st->mask_ok;
    const MaskOp& mo = st->maskop;
    auto rows = [&](int r0, int r1, int grid) {
        a.row0 = r0;
        a.row1 = r1;
        if (p.sweep_queued) {
            push_phase(ctx, st, PH_SMOOTH, lv.N).u.s = a;
        } else if (!mask) {
            launch_smooth(ctx, a, grid);
        } else {
            const size_t dyn = sizeof(double) * 64 * (size_t)std::max(mo.nwf, mo.nwc);
            const int nwh = (r0 < mo.nf) ? mo.nwf : mo.nwc;
            const int mgrid = std::max(1, cdiv(r1 - r0, std::min(MASK_RW, 64 / nwh) * (BT / 64)));
            hipLaunchKernelGGL(k_smooth_mask, dim3(mgrid), dim3(BT), dyn, ctx->stream, a, mo);
            IPD_KERNEL_CHECK();
        }
    };
    // Jacobi: one range.  Bigraph GS: the first half hands its result (wout) to the second, which updates with it
    const HalfRanges& hr = p.sweep[post ? 1 : 0];
    a.u0 = a.u1 = 0;
    for (int i = 0; i < hr.n; ++i) {
        if (i == hr.n - 1) a.wout = nullptr;
        if (p.sweep_queued)
            rows(hr.r[i].r0, hr.r[i].r1, 0);
        else
            run_rows(ctx, st, hr.r[i], a.lv.L, rows, {a.enew, a.wout});
        a.u0 = hr.r[i].r0;
        a.u1 = hr.r[i].r1;
    }
    rn.e_zero = false;
    std::swap(lv.e, lv.e2);
}

__global__ void k_maskop_scales(int nf, int nc, const double* __restrict__ p,
                                const double* __restrict__ q, double itk,
                                double* __restrict__ alpha, double* __restrict__ beta) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nf + nc; t += gridDim.x * blockDim.x) {
        if (t < nf)
            alpha[t] = q[t] * q[t] * itk;
        else
            beta[t - nf] = p[t - nf] * p[t - nf];
    }
}

void launch_subcycle(ipd_ctx* ctx, CycleState* st, bool keep_e) {
    hipLaunchKernelGGL(k_subcycle, dim3(1), dim3(BT), st->img[IMG_SUB].lds, ctx->stream,
                       (const SolveDesc*)st->img[IMG_SUB].desc, keep_e ? 1 : 0);
    IPD_KERNEL_CHECK();
}

// Solves A_k e = r_k approximately; r in L[k].r, result in L[k].e.
// keep_e: start from the current L[k].e (second leg of a W cycle); otherwise the
// start is e = 0, which is never materialised (the first sweep does not read it).
void amg_cycle(ipd_amg* h, int k, int isnsp, bool wcycle, bool keep_e) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    Level& lv = h->L[k];
    LevelRun& rn = st->run[(size_t)k];
    const LaunchLevel& p = rn.plan;
    if (st->k_sub == k) {  // everything from here down: one workgroup, LDS-resident (replicated)
        flush_fused(ctx, st);
        launch_subcycle(ctx, st, keep_e);
        rn.e_zero = false;
        return;
    }
    if (k == h->J) {                                   // MG_Vcycle.m:43 / MG_Wcycle.m:44
        PcgArgs a = rn.pcg;                            // replicated on every rank
        a.rhs = lv.r;
        a.d = lv.e;
        push_phase(ctx, st, PH_PCG, 0).u.p = a;
        return;
    }
    const int nu = h->opts.smoth;
    if (!keep_e) {
        rn.e_zero = true;
        if (nu == 0) {  // no sweep will overwrite the iterate: materialise the zero
            flush_fused(ctx, st);
            IPD_HIP(hipMemsetAsync(lv.e, 0, sizeof(double) * (size_t)lv.N, ctx->stream));
            rn.e_zero = false;
        }
    }
    for (int s = 0; s < nu; ++s) launch_sweep(h, st, k, isnsp, false);          // :14-25
    XferArgs ra = rn.restrict_args;
    if (p.rrc) {
        // r_{k+1} = P'r - (P'A) e: one launch instead of residual + restriction           :27
        const Csr& T1 = h->L[k + 1].T1;
        RrcArgs rc;
        rc.p = ra;
        rc.p.x = lv.r;
        rc.p.L = p.rrc_walk.L;
        rc.rp2 = T1.rp;
        rc.ci2 = T1.ci;
        rc.va2 = T1.va;
        rc.e = lv.e;
        const bool staged = p.rrc_walk.staged;
        const size_t dyn = staged ? 2 * sizeof(double) * (size_t)ra.ncols : 0;
        run_rows(ctx, st, RowRange{0, ra.nrows, p.rrc_walk.G}, rc.p.L,
                 [&](int r0, int r1, int grid) {
                     rc.p.row0 = r0;
                     rc.p.row1 = r1;
                     if (staged)
                         hipLaunchKernelGGL(k_rrc<true>, dim3(grid), dim3(BT), dyn, ctx->stream, rc);
                     else
                         hipLaunchKernelGGL(k_rrc<false>, dim3(grid), dim3(BT), 0, ctx->stream, rc);
                     IPD_KERNEL_CHECK();
                 },
                 {ra.y});
    } else {
        if (p.resid_queued) {                                                           // :27
            ResidDesc& rd = push_phase(ctx, st, PH_RESID, lv.N).u.r;
            rd.lv = rn.dev;
            rd.e = lv.e;
            rd.row0 = 0;
            rd.row1 = lv.N;
        } else {
            run_rows(ctx, st, RowRange{0, lv.N, p.G_all}, rn.dev.L,
                     [&](int r0, int r1, int grid) { launch_resid(ctx, rn, lv.e, r0, r1, grid); }, {lv.rr});
        }
        issue_xfer(ctx, st, ra, p.rest);
    }
    amg_cycle(h, k + 1, isnsp, wcycle, false);                                   // :29
    // MG_Wcycle.m:30 -- the second correction; on the coarsest level it repeats the
    // identical zero-guess PCG solve, so it is skipped there (same bits).
    if (wcycle && k + 1 < h->J) amg_cycle(h, k + 1, isnsp, wcycle, true);
    XferArgs pa = rn.prolong_args;                                               // :31
    pa.x = h->L[k + 1].e;
    pa.y = lv.e;
    issue_xfer(ctx, st, pa, p.prol);
    for (int s = 0; s < nu; ++s) launch_sweep(h, st, k, isnsp, true);           // :33-41
}

void launch_top(ipd_amg* h, CycleState* st, const double* b, const double* x,
                       const double* e, double* xnew, bool first) {
    ipd_ctx* ctx = h->ctx;
    LevelRun& rn = st->run[1];
    TopArgs a;
    a.lv = rn.dev;
    a.b = b;
    a.x = x;
    a.e = e;
    a.xnew = xnew;
    a.staged = rn.plan.staged;
    const size_t dyn = a.staged ? sizeof(double) * (size_t)rn.dev.N : 0;
    if (rn.plan.top_queued) {
        a.row0 = 0;
        a.row1 = rn.dev.N;
        push_phase(ctx, st, PH_TOP, rn.dev.N).u.t = a;
    } else {
        run_rows(ctx, st, RowRange{0, rn.dev.N, rn.plan.G_all}, rn.dev.L,
                 [&](int r0, int r1, int grid) {
                     a.row0 = r0;
                     a.row1 = r1;
                     dispatch_staged_pad(a.staged, rn.dev.S > 0, [&](auto S, auto P) {
                         hipLaunchKernelGGL((k_top<decltype(S)::value, decltype(P)::value>), dim3(grid), dim3(BT), decltype(S)::value ? dyn : 0, ctx->stream, a);
                     });
                     IPD_KERNEL_CHECK();
                 },
                 {rn.dev.r, xnew});
    }
    ConvArgs ca;
    ca.r = rn.dev.r;
    ca.n = rn.dev.N;
    ca.hist = st->hist;
    ca.first = first ? 1 : 0;
    push_phase(ctx, st, PH_CONV, 0).u.c = ca;
    flush_fused(ctx, st);  // the loop body ends here: nothing stays queued across calls
}

// one Class_AMG loop body (Class_AMG.m:96-105): x_out = x_in + cycle(b - A x_in)
void enqueue_loop_body(ipd_amg* h, CycleState* st, const double* b, const double* xin,
                              double* xout) {
    const bool wc = h->opts.cycle == 'w', vc = h->opts.cycle == 'v';
    const double* ecorr = nullptr;
    if (vc || wc) {
        amg_cycle(h, 1, h->opts.isnsp, wc, false);
        ecorr = h->L[1].e;
    }
    launch_top(h, st, b, xin, ecorr, xout, false);
}

// the whole solve phase (cycles == 0) or `cycles` cycles without stopping rules as one single-workgroup launch
void launch_solve_small(ipd_ctx* ctx, CycleState* st, const double* b_dev, double* x, int cycles) {
    const CycleState::Image& im = st->img[IMG_SOLVE];
    if (st->solve_cached)
        hipLaunchKernelGGL(k_solve_small<true>, dim3(1), dim3(BT), im.lds, ctx->stream, (const SolveDesc*)im.desc,
                           b_dev, x, st->x2, st->hist, st->solve_out, cycles);
    else
        hipLaunchKernelGGL(k_solve_small<false>, dim3(1), dim3(BT), im.lds, ctx->stream, (const SolveDesc*)im.desc,
                           b_dev, x, st->x2, st->hist, st->solve_out, cycles);
    IPD_KERNEL_CHECK();
}

static void copy_vec(ipd_ctx* ctx, double* dst, const double* src, int N) {
    IPD_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
}

// x = the initial guess (NULL: zeros)
static void load_guess(ipd_ctx* ctx, double* x, const double* guess_dev, int N) {
    if (guess_dev)
        copy_vec(ctx, x, guess_dev, N);
    else
        IPD_HIP(hipMemsetAsync(x, 0, sizeof(double) * (size_t)N, ctx->stream));
}

// Class_AMG.m:86-109
void amg_solve_dev(ipd_amg* h, const double* b_dev, const double* guess_dev, double* x_dev,
                   int32_t* it_out, double* rel_res_out, double* rel_resk, double* rhok) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    const AmgOpts& o = h->opts;
    const int N = h->L[1].A.nr;
    double* xa = h->x;
    double* xb = st->x2;
    load_guess(ctx, xa, guess_dev, N);
    // what a one-launch solve read back: iterations, last relative residual, then the two histories
    auto deliver = [&](const std::vector<double>& out) {
        const int its = (int)out[0];
        if (rel_resk) std::memcpy(rel_resk, out.data() + 4, sizeof(double) * ((size_t)its + 1));
        if (rhok) std::memcpy(rhok, out.data() + 4 + (o.maxit + 2), sizeof(double) * ((size_t)its + 1));
        if (x_dev) copy_vec(ctx, x_dev, xa, N);
        if (it_out) *it_out = its;
        if (rel_res_out) *rel_res_out = out[1];
        ctx->sync();
    };
    if (st->small_ok && st->shard_ranks == 1) {
        // small hierarchy: the whole solve phase is one single-workgroup launch
        launch_solve_small(ctx, st, b_dev, xa, 0);
        const size_t nout = 4 + 2 * ((size_t)o.maxit + 2);
        std::vector<double> out(nout);
        ctx->fetch(st->solve_out, out.data(), nout);
        deliver(out);
        return;
    }
    if (resident_active(st) && st->shard_ranks == 1) {
        // dense regime: the whole solve phase is one launch of co-resident workgroups
        std::vector<double> out;
        if (run_resident(h, st, b_dev, xa, 0, &out, nullptr)) {
            deliver(out);
            return;
        }
        // not usable right now: restore the initial guess and take the multi-launch path
        load_guess(ctx, xa, guess_dev, N);
    }
    launch_top(h, st, b_dev, xa, nullptr, xb, true);                            // :89
    std::swap(xa, xb);
    double hh[5];
    ctx->fetch(st->hist, hh, 5);
    int it = 0;
    double rel_res = 0.0;
    if (hh[0] == 0.0) {                                                          // :91-92
        if (rel_resk) rel_resk[0] = 0.0;
        if (rhok) rhok[0] = INFINITY;
    } else {
        it = 1;                                                                  // :94
        double last_rel = 1.0;
        if (rel_resk) rel_resk[0] = 1.0;
        if (rhok) rhok[0] = NAN;
        while (last_rel > o.retol && it <= o.maxit) {                            // :95
            enqueue_loop_body(h, st, b_dev, xa, xb);                             // :96-105
            std::swap(xa, xb);
            ctx->fetch(st->hist, hh, 5);
            rel_res = hh[3];
            last_rel = rel_res;
            if (rel_resk) rel_resk[it] = rel_res;
            if (rhok) rhok[it] = hh[4];
            ++it;
            if (hh[4] > 1.0) break;                                              // :106
        }
        it -= 1;                                                                 // :108
    }
    if (x_dev) copy_vec(ctx, x_dev, xa, N);
    if (xa != h->x) std::swap(h->x, st->x2);  // keep h->x pointing at the current iterate
    if (it_out) *it_out = it;
    if (rel_res_out) *rel_res_out = rel_res;
    ctx->sync();
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_amg_solve_dev(ipd_amg* h, const double* b_dev, const double* guess_dev,
                                 double* x_dev, int32_t* it, double* rel_res, double* rel_resk,
                                 double* rhok) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b_dev && x_dev, IPD_E_ARG, "NULL argument");
        CallScope scope(h->ctx);
        amg_solve_dev(h, b_dev, guess_dev, x_dev, it, rel_res, rel_resk, rhok);
    });
}

extern "C" int ipd_amg_solve(ipd_amg* h, const double* b, const double* guess, double* x,
                             int32_t* it, double* rel_res, double* rel_resk, double* rhok) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b && x, IPD_E_ARG, "NULL argument");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        const size_t N = (size_t)h->L[1].A.nr;
        double* db = ctx->scratch->alloc<double>(N);
        double* dg = nullptr;
        double* dx = ctx->scratch->alloc<double>(N);
        ctx->upload(db, b, N);
        if (guess) {
            dg = ctx->scratch->alloc<double>(N);
            ctx->upload(dg, guess, N);
        }
        amg_solve_dev(h, db, dg, dx, it, rel_res, rel_resk, rhok);
        ctx->fetch(dx, x, N);
    });
}

static void run_cycle_api(ipd_amg* h, const double* r, int isnsp, int k, const double* e_in,
                          double* e_out, bool wc) {
    IPD_REQUIRE(h && r && e_out, IPD_E_ARG, "NULL argument");
    IPD_REQUIRE(k >= 1 && k <= h->J, IPD_E_ARG, "level k out of range");
    ipd_ctx* ctx = h->ctx;
    CallScope scope(ctx);
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    Level& lv = h->L[k];
    const size_t N = (size_t)lv.A.nr;
    ctx->upload(lv.r, r, N);
    LevelRun& rn = st->run[(size_t)k];
    bool keep = false;
    if (e_in && wc) {  // MG_Wcycle(r,isnsp,k,e): start from the caller's iterate
        ctx->upload(lv.e, e_in, N);
        rn.e_zero = false;
        keep = true;
    }
    amg_cycle(h, k, isnsp, wc, keep);
    flush_fused(ctx, st);
    ctx->fetch(h->L[k].e, e_out, N);
}

// ---- the cycle as a preconditioner (ipd_krylov.hip) -------------------------------------
bool amg_level1_walk(ipd_amg* h, LevelDev* lv, int* staged, int* grid) {
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    if (st->shard_ranks > 1 && !st->shard_emulate) return false;
    const LevelRun& rn = st->run[1];
    *lv = rn.dev;
    *staged = rn.plan.staged ? 1 : 0;
    *grid = rn.plan.G_all;
    return true;
}

// ---- the launch-path cycle's CSR forms, for the block solve (ipd_block.hip) ----------------
bool amg_block_levels(ipd_amg* h, std::vector<BlockLevel>* out) {
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    if (st->shard_ranks > 1) return false;
    if (!out) return true;
    auto csr_of = [](const Csr& m, int L, int grid) { return BlockCsr{m.nr, m.nc, L, grid, m.rp, m.ci, m.va}; };
    out->assign((size_t)h->J + 1, BlockLevel{});
    for (int k = 1; k <= h->J; ++k) {
        const Level& lv = h->L[k];
        const LevelRun& rn = st->run[(size_t)k];
        BlockLevel& bl = (*out)[(size_t)k];
        bl.N = lv.N;
        bl.nf = lv.nf;
        const LaunchLevel& p = rn.plan;
        bl.A = csr_of(lv.A, p.L, p.G_all);
        bl.sweep[0] = p.sweep[0];
        bl.sweep[1] = p.sweep[1];
        bl.dinv = lv.dinv;
        bl.Axi = lv.Axi;
        bl.xx = lv.xx;
        if (k < h->J) {
            const Level& cl = h->L[k + 1];
            bl.Pt = csr_of(cl.Pt, p.rest.L, p.rest.G);
            bl.P = csr_of(cl.P, p.prol.L, p.prol.G);
            if (p.rrc_rule) bl.T1 = csr_of(cl.T1, p.rrc_walk.L, p.rrc_walk.G);
        } else {
            const PcgArgs& a = rn.pcg;
            bl.pcg_L = a.L;
            bl.pcg_precd = a.precd;
            bl.pcg_tol = a.tol;
            bl.pcg_maxit = a.maxit;
        }
    }
    return true;
}

void amg_apply_cycle(ipd_amg* h) {
    const int cyc = h->opts.cycle;
    IPD_REQUIRE(cyc == 'v' || cyc == 'w', IPD_E_ARG, "AMG-PCG: the hierarchy's cycle must be 'v' or 'w'");
    amg_cycle(h, 1, h->opts.isnsp, cyc == 'w', false);   // what run_cycle_api(h, r, isnsp, 1, NULL, ..) runs
    flush_fused(h->ctx, state_of(h));
}

// ---- the whole AMG-PCG solve as one single-workgroup launch (ipd_amg_pcg_planned) ---------
bool amg_pcg_small_ok(ipd_amg* h) {
    CycleState* st = state_of(h);
    IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
    return st->small_ok && st->shard_ranks == 1;
}

void amg_pcg_small_launch(ipd_amg* h, const PcgSmallVecs& v, double tol, int maxit) {
    ipd_ctx* ctx = h->ctx;
    CycleState* st = state_of(h);
    IPD_REQUIRE(st && st->small_ok && st->shard_ranks == 1, IPD_E_ARG,
                "AMG-PCG: the hierarchy is not planned for the single-workgroup solve");
    IPD_REQUIRE(maxit >= 0 && maxit <= PCG_SMALL_MAXIT, IPD_E_ARG, "AMG-PCG: maxit beyond the one-launch cap");
    PcgSmallArgs a;
    a.e = v.e;
    a.d = v.d;
    a.r = v.r;
    a.p = v.p;
    a.q = v.q;
    a.w_old = v.w_old;
    a.tol2 = tol * tol;
    a.maxit = maxit;
    a.out = v.out;
    if (st->solve_cached)
        hipLaunchKernelGGL(k_pcg_small<true>, dim3(1), dim3(BT), st->img[IMG_SOLVE].lds, ctx->stream,
                           (const SolveDesc*)st->img[IMG_SOLVE].desc, a);
    else
        hipLaunchKernelGGL(k_pcg_small<false>, dim3(1), dim3(BT), st->img[IMG_SOLVE].lds, ctx->stream,
                           (const SolveDesc*)st->img[IMG_SOLVE].desc, a);
    IPD_KERNEL_CHECK();
}

extern "C" int ipd_amg_vcycle(ipd_amg* h, const double* r, int isnsp, int k, double* e) {
    return ipd_guard([&] { run_cycle_api(h, r, isnsp, k, nullptr, e, false); });
}

extern "C" int ipd_amg_wcycle(ipd_amg* h, const double* r, int isnsp, int k, const double* e_in,
                              double* e_out) {
    return ipd_guard([&] { run_cycle_api(h, r, isnsp, k, e_in, e_out, true); });
}

extern "C" int ipd_class_amg(ipd_ctx* ctx, const ipd_csc* A, const double* b, const double* guess,
                             const ipd_amg_opts* o, ipd_rng* rng, double* x, int32_t* it,
                             double* rel_res, double* rel_resk, double* rhok) {
    ipd_amg* h = nullptr;
    int rc = ipd_amg_setup(ctx, A, o, rng, &h);
    if (rc != IPD_OK) return rc;
    rc = ipd_amg_solve(h, b, guess, x, it, rel_res, rel_resk, rhok);
    ipd_amg_destroy(h);
    return rc;
}

extern "C" int ipd_pcg(ipd_ctx* ctx, const ipd_csc* H, const double* e, const double* guess,
                       const ipd_pcg_opts* o, double* d, int64_t* it, double* res, double* resk) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && H && e && d, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        Arena& tmp = *ctx->scratch;
        double tol = 1e-11;
        long long maxit = 10000;
        int precd = 2;  // PCG.m:24-27 defaults
        long long nf = 0;
        if (o) {
            if (o->retol >= 0) tol = o->retol;
            if (o->maxit >= 0) maxit = o->maxit;
            if (o->precd >= 0) precd = o->precd;
            nf = o->nf;
        }
        Csr hm;
        csr_upload_from_csc(ctx, tmp, H, false, &hm);  // true rows of H
        const size_t N = (size_t)hm.nr;
        double* de = tmp.alloc<double>(N);
        double* dd = tmp.alloc<double>(N);
        double* dg = nullptr;
        ctx->upload(de, e, N);
        if (guess) {
            dg = tmp.alloc<double>(N);
            ctx->upload(dg, guess, N);
        }
        long long its = 0;
        pcg_dev(ctx, hm, de, dg, tol, maxit, precd, dd, &its, res, resk, nf);
        if (it) *it = its;
        ctx->fetch(dd, d, N);
    });
}

// How the levels held in the LDS images of this hierarchy run (bit mask over all images packed):
// 1 thread-per-row sweeps, 2 the same with dense rows in registers, 4 one-wave sweeps, 8 one-wave
// polynomial form, 16 block-wide polynomial form; 0: the level is in no image.
extern "C" int ipd_amg_level_forms(const ipd_amg* h, int32_t* forms, int32_t count) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && forms && count >= 0, IPD_E_ARG, "bad argument");
        const CycleState* st = h->cyc.get();
        for (int k = 0; k < count; ++k)
            forms[k] = (st && (size_t)k < st->level_forms.size()) ? st->level_forms[(size_t)k] : 0;
    });
}

// Test hook: the block-wide polynomial operator of level k as packed for the images, column-major with
// *ld rows: columns [Mr (N8) | Me (N8) | Mc (Nc8)] then the column W (N8 = N rounded up to 8); needs
// ld * (2 N8 + Nc8 + 1) doubles.  IPD_E_ARG when level k has no such operator.
extern "C" int ipd_amg_poly_operator(const ipd_amg* h, int32_t k, double* out, int64_t cap, int32_t* ld,
                                     int32_t* n, int32_t* nc) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && out && ld && n && nc, IPD_E_ARG, "NULL argument");
        const CycleState* st = h->cyc.get();
        IPD_REQUIRE(st && k >= 1 && (size_t)k < st->poly_ops.size() && st->poly_ops[(size_t)k].M, IPD_E_ARG,
                    "level has no block-wide polynomial operator");
        const CycleState::PolyOp& po = st->poly_ops[(size_t)k];
        const int64_t N8 = (po.N + 7) / 8 * 8, Nc8 = (po.Nc + 7) / 8 * 8;
        const int64_t need = (int64_t)po.LD * (2 * N8 + Nc8 + 1);
        IPD_REQUIRE(cap >= need, IPD_E_ARG, "buffer too small");
        h->ctx->fetch(po.M, out, (size_t)need);   // W lies right behind M (pack_bpoly)
        *ld = po.LD;
        *n = po.N;
        *nc = po.Nc;
    });
}

// Test hook: the polynomial operator of level k exactly as packed for `form` (see include/ipd_amg.h).
extern "C" int ipd_amg_packed_operator(const ipd_amg* h, int32_t k, int32_t form, double* out, int64_t cap,
                                       int32_t* ld, int32_t* seg, int32_t* n, int32_t* nc) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && ld && seg && n && nc && (out || cap == 0), IPD_E_ARG, "NULL argument");
        const CycleState* st = h->cyc.get();
        IPD_REQUIRE(st && (form == 16 || form == 64 || form == 128), IPD_E_ARG, "no such form");
        const double* M = nullptr;
        int LD = 0, S = 0, N = 0, Nc = 0;
        int64_t need = 0;
        if (form == 16) {
            if (k >= 1 && (size_t)k < st->poly_ops.size()) {
                const CycleState::PolyOp& po = st->poly_ops[(size_t)k];
                M = po.M;
                LD = po.LD;
                N = po.N;
                Nc = po.Nc;
                S = (N + 7) / 8 * 8;
                need = (int64_t)LD * (2 * S + (Nc + 7) / 8 * 8 + 1);   // W lies right behind M (pack_bpoly)
            }
        } else {
            const CycleState::RowsOp* op = nullptr;
            if (form == 64 && k >= 1 && (size_t)k < st->rows_ops.size()) op = &st->rows_ops[(size_t)k];
            if (form == 128 && k == 2) op = &st->poly2_op;
            if (op) {
                M = op->M;
                LD = op->ld;
                S = op->seg;
                N = op->N;
                Nc = op->Nc;
                need = (int64_t)(N + Nc) * (LD + 1);                   // W lies right behind the rows
            }
        }
        IPD_REQUIRE(M, IPD_E_ARG, "level has no operator packed in that form");
        *ld = LD;
        *seg = S;
        *n = N;
        *nc = Nc;
        if (!out) return;   // size query
        IPD_REQUIRE(cap >= need, IPD_E_ARG, "buffer too small");
        h->ctx->fetch(M, out, (size_t)need);
    });
}
