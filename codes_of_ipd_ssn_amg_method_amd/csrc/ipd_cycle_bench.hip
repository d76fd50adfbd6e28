// Measurement hooks of the cycle: timed loop bodies (eager or as captured graphs), timed sub-cycles and sweeps, the
// sharded loop body, and the byte count of a cycle.  No kernel of its own.
#include "ipd_cycle_state.h"

#include <cmath>

static void copy_vec(ipd_ctx* ctx, double* dst, const double* src, int N) {
    IPD_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
}

// Times what the stream is given between construction and stop() with HIP events
struct StreamTimer {
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit StreamTimer(hipStream_t s) : stream(s) {
        IPD_HIP(hipEventCreate(&e0));
        IPD_HIP(hipEventCreate(&e1));
        IPD_HIP(hipEventRecord(e0, stream));
    }
    float stop() {   // milliseconds
        IPD_HIP(hipEventRecord(e1, stream));
        IPD_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        IPD_HIP(hipEventElapsedTime(&ms, e0, e1));
        return ms;
    }
    ~StreamTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// ---------------------------------------------------------------------------
// measurement hooks
// ---------------------------------------------------------------------------
// S(X) = 12 nnz + 4 (rows+1) + 8 rows + 8 cols per CSR SpMV.
static double spmv_bytes(const Csr& m) {
    return 12.0 * m.nnz + 4.0 * (m.nr + 1) + 8.0 * m.nr + 8.0 * m.nc;
}

// B_V with the fused Gauss-Seidel form (one S(A_1) per level-1 sweep, the stated
// minimum): per level (2 nu + 1) S(A_k) + S(P) + S(P') + 6 nu 8 N_k, weighted by
// the visit count (1 for V, 2^(k-1) for W), + coarsest PCG + the outer loop's
// residual S(A_1) + 32 M.
static double cycle_bytes(const ipd_amg* h) {
    const bool wc = h->opts.cycle == 'w';
    const double nu = h->opts.smoth;
    double total = 0.0;
    double visits = 1.0;
    for (int k = 1; k < h->J; ++k) {
        const Level& lv = h->L[k];
        const Level& cl = h->L[k + 1];
        const double per = (2 * nu + 1) * spmv_bytes(lv.A) + spmv_bytes(cl.P) + spmv_bytes(cl.Pt) +
                           6 * nu * 8.0 * lv.A.nr;
        total += visits * per;
        if (wc && k + 1 < h->J) visits *= 2.0;
    }
    total += visits * 2.0 * spmv_bytes(h->L[h->J].A);  // >= 1 PCG iteration + initial residual
    total += spmv_bytes(h->L[1].A) + 32.0 * h->L[1].A.nr;
    return total;
}

extern "C" int ipd_amg_cycle_bytes(const ipd_amg* h, double* bytes_per_cycle) {
    if (!h || !bytes_per_cycle) return IPD_E_ARG;
    *bytes_per_cycle = cycle_bytes(h);
    return IPD_OK;
}

// Captures the two loop bodies (x -> x2 and x2 -> x) as HIP graphs: one graph launch
// per cycle instead of ~40 kernel launches, so the host never paces the device.
static void ensure_graphs(ipd_amg* h, CycleState* st, const double* b_dev) {
    if (st->gexec[0] && st->gb == b_dev) return;
    ipd_ctx* ctx = h->ctx;
    for (auto& g : st->gexec)
        if (g) {
            IPD_HIP(hipGraphExecDestroy(g));
            g = nullptr;
        }
    double* xs[2] = {h->x, st->x2};
    for (int v = 0; v < 2; ++v) {
        hipGraph_t graph = nullptr;
        IPD_HIP(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        try {
            enqueue_loop_body(h, st, b_dev, xs[v], xs[v ^ 1]);
        } catch (...) {
            (void)hipStreamEndCapture(ctx->stream, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            throw;
        }
        IPD_HIP(hipStreamEndCapture(ctx->stream, &graph));
        hipError_t e = hipGraphInstantiate(&st->gexec[v], graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        IPD_HIP(e);
    }
    st->gb = b_dev;
}

// Times `cycles` loop bodies on x_dev, eager or as the captured graphs, after the initial residual
// (Class_AMG.m:89); milliseconds
static float time_loop_bodies(ipd_amg* h, CycleState* st, const double* b_dev, double* x_dev, int cycles,
                              bool use_graph) {
    ipd_ctx* ctx = h->ctx;
    const int N = h->L[1].A.nr;
    copy_vec(ctx, h->x, x_dev, N);
    launch_top(h, st, b_dev, h->x, nullptr, st->x2, true);   // x stays in h->x
    copy_vec(ctx, h->x, st->x2, N);
    if (use_graph) ensure_graphs(h, st, b_dev);
    double* xs[2] = {h->x, st->x2};
    StreamTimer timer(ctx->stream);
    int v = 0;
    for (int c = 0; c < cycles; ++c) {
        if (use_graph)
            IPD_HIP(hipGraphLaunch(st->gexec[v], ctx->stream));
        else
            enqueue_loop_body(h, st, b_dev, xs[v], xs[v ^ 1]);
        v ^= 1;
    }
    const float ms = timer.stop();
    copy_vec(ctx, x_dev, xs[v], N);
    return ms;
}

extern "C" int ipd_amg_bench_cycles(ipd_amg* h, const double* b_dev, double* x_dev, int cycles,
                                    double* total_ms, double* bytes_per_cycle) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b_dev && x_dev && cycles > 0 && total_ms, IPD_E_ARG, "bad argument");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        CycleState* st = state_of(h);
        IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
        const int N = h->L[1].A.nr;
        float ms = 0.f;
        bool done = false;
        if (st->small_ok || resident_active(st)) {  // one launch runs all the cycles (no stopping rules)
            copy_vec(ctx, h->x, x_dev, N);
            if (st->small_ok) {            // ... of one workgroup
                StreamTimer timer(ctx->stream);
                launch_solve_small(ctx, st, b_dev, h->x, cycles);
                ms = timer.stop();
                done = true;
            } else {                       // ... of co-resident workgroups
                done = run_resident(h, st, b_dev, h->x, cycles, nullptr, &ms);
            }
            if (done) copy_vec(ctx, x_dev, h->x, N);
        }
        if (!done) ms = time_loop_bodies(h, st, b_dev, x_dev, cycles, !switch_on("IPD_NO_GRAPH"));
        ctx->sync();
        *total_ms = ms;
        if (bytes_per_cycle) *bytes_per_cycle = cycle_bytes(h);
    });
}

// Times `reps` launches of the sub-cycle kernel on the IMG_SUB image with HIP events; stamps: its stage clocks
extern "C" int ipd_amg_bench_subcycle(ipd_amg* h, int reps, double* total_ms, int32_t* k_sub,
                                      int64_t stamps[8]) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && reps > 0 && total_ms, IPD_E_ARG, "bad argument");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        CycleState* st = state_of(h);
        IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
        if (k_sub) *k_sub = st->k_sub;
        *total_ms = 0.0;
        if (!st->k_sub) return;
        CallScope scope(ctx);
        long long* dbg = ctx->scratch->alloc<long long>(16);
        IPD_HIP(hipMemsetAsync(dbg, 0, 128, ctx->stream));
        // patch the debug pointer into the image header
        const size_t off = offsetof(SolveDesc, dbg);
        // (a stamp is two s_memrealtime reads and a read-modify-write of global memory, ~0.5 us each: the
        // per-stage figures are for proportions)
        ctx->upload_bytes(reinterpret_cast<char*>(st->img[IMG_SUB].desc) + off, &dbg, sizeof(dbg));
        {   // a right-hand side that is not zero (a zero one ends every coarse PCG at once)
            std::vector<double> rr((size_t)h->L[st->k_sub].N);
            unsigned lcg = 12345u;
            for (auto& v : rr) {
                lcg = lcg * 1664525u + 1013904223u;
                v = (double)(lcg >> 8) / (double)(1u << 24) - 0.5;
            }
            ctx->upload(h->L[st->k_sub].r, rr.data(), rr.size());
        }
        launch_subcycle(ctx, st, false);
        StreamTimer timer(ctx->stream);
        for (int r = 0; r < reps; ++r) launch_subcycle(ctx, st, false);
        const float ms = timer.stop();
        *total_ms = ms;
        long long hs[16];
        ctx->fetch(dbg, hs, 16);
        if (stamps && hs[3] > hs[2])   // shader clock (MHz) seen by the cycle: s_memtime ticks / 10 ns
            stamps[0] = hs[8] * 100 / (hs[3] - hs[2]), hs[0] = stamps[0];
        if (stamps)
            for (int i = 0; i < 8; ++i) stamps[i] = hs[i];
        long long* none = nullptr;
        ctx->upload_bytes(reinterpret_cast<char*>(st->img[IMG_SUB].desc) + off, &none, sizeof(none));
    });
}

// Times `reps` smoother sweeps of level k (pre-smoothing direction) with HIP events on
// the context's stream: the per-launch duration of the dominant kernel (k_smooth).
// launches_per_sweep = 2 for the bigraph Gauss-Seidel level, 1 for Jacobi levels;
// bytes_per_sweep = S(A_k) + 6*8*N_k (fused-GS form).
extern "C" int ipd_amg_bench_sweeps(ipd_amg* h, int k, int reps, double* total_ms,
                                    int* launches_per_sweep, double* bytes_per_sweep) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && total_ms && reps > 0, IPD_E_ARG, "bad argument");
        IPD_REQUIRE(k >= 1 && k < h->J, IPD_E_ARG, "level must be a smoothed level (1 <= k < J)");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        CycleState* st = state_of(h);
        Level& lv = h->L[k];
        LevelRun& rn = st->run[(size_t)k];
        fill_f64(ctx, lv.r, 1.0, (size_t)lv.N);
        rn.e_zero = true;
        for (int w = 0; w < 4; ++w) launch_sweep(h, st, k, h->opts.isnsp, false);
        flush_fused(ctx, st);
        StreamTimer timer(ctx->stream);
        for (int s = 0; s < reps; ++s) launch_sweep(h, st, k, h->opts.isnsp, false);
        flush_fused(ctx, st);
        const float ms = timer.stop();
        *total_ms = ms;
        if (launches_per_sweep) *launches_per_sweep = lv.nf > 0 ? 2 : 1;
        if (bytes_per_sweep) *bytes_per_sweep = spmv_bytes(lv.A) + 6 * 8.0 * lv.A.nr;
    });
}

// Row-block sharded loop body (eager launches; RCCL calls are not graph-captured).
extern "C" int ipd_amg_bench_cycles_sharded(ipd_amg* h, const double* b_dev, double* x_dev,
                                            int cycles, double* total_ms,
                                            double* bytes_per_cycle) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && b_dev && x_dev && cycles > 0 && total_ms, IPD_E_ARG, "bad argument");
        ipd_ctx* ctx = h->ctx;
        CallScope scope(ctx);
        CycleState* st = state_of(h);
        IPD_REQUIRE(st, IPD_E_ARG, "hierarchy has no cycle state");
        const char* emu = switch_value("IPD_SHARD_EMULATE");
        const int emu_ranks = emu ? std::atoi(emu) : 0;
        struct Restore {
            CycleState* st;
            ~Restore() {
                st->shard_ranks = 1;
                st->shard_rank = 0;
                st->shard_emulate = false;
            }
        } restore{st};
        if (emu_ranks > 1) {
            st->shard_ranks = emu_ranks;
            st->shard_emulate = true;
        } else {
            st->shard_ranks = comm_size(ctx);
            st->shard_rank = comm_rank(ctx);
            IPD_REQUIRE(st->shard_ranks == 1 || ctx->comm, IPD_E_COMM, "call ipd_comm_init first");
        }
        const float ms = time_loop_bodies(h, st, b_dev, x_dev, cycles, false);
        ctx->sync();
        *total_ms = ms;
        if (bytes_per_cycle) *bytes_per_cycle = cycle_bytes(h);
    });
}
