// Host rules of AMG-PCG, its multi-right-hand-side form and the block solve (ipd_krylov.hip, ipd_block.hip,
// ipd_block_krylov.hip), each written once: block width and chunking of nrhs, LDS staging of a block, the grids,
// the pcg_options rule, the route of ipd_amg_pcg_planned and the indexing of the host histories.  The executors
// call these and compare no size against a threshold.  Host-clean, no HIP, no getenv: tests/krylov_plan_driver.cpp
// runs it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <type_traits>

#include "ipd_amg.h"           // ipd_pcg_opts
#include "ipd_launch_plan.h"   // stage_fits
#include "ipd_limits.h"

static inline int kry_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// columns of the block that n right-hand sides run in: the next power of two, at most BLK_WMAX
static inline int block_width(long long n) {
    int W = 1;
    while (W < n && W < BLK_WMAX) W <<= 1;
    return W;
}

// f(std::integral_constant<int, W>) for a run-time block width: the one switch over the instantiated widths
template <class F>
static inline void with_block_width(int W, F&& f) {
    switch (W) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, BLK_WMAX>{}); break;
    }
}

// f(j0, ncol, W) for every chunk of at most BLK_WMAX columns of a call, in order
template <class F>
static inline void block_chunks(long long nrhs, F&& f) {
    for (long long j0 = 0; j0 < nrhs; j0 += BLK_WMAX) {
        const int ncol = (int)std::min<long long>(BLK_WMAX, nrhs - j0);
        f(j0, ncol, block_width(ncol));
    }
}

// a gathered block of len rows x W columns goes through LDS (dyn bytes) or is gathered from L2
struct BlockStage {
    bool staged;
    size_t dyn;
};
static inline BlockStage block_stage(long long len, int W) {
    const bool staged = stage_fits(len * W);
    return {staged, staged ? sizeof(double) * (size_t)len * W : 0};
}

// workgroups of the vector passes K2 and K3 of a PCG iteration (K1 takes level 1's row-walk grid)
static inline int krylov_g3(int N, int num_cu) { return std::max(1, std::min(num_cu, kry_cdiv(N, BT))); }

// workgroups of k_blk_in / k_blk_out (BLK_IO_BT threads each, grid-stride)
static constexpr int BLK_IO_BT = 256;
static inline int block_io_grid(long long N, int W) { return std::max(1, std::min(1024, kry_cdiv(N * W, BLK_IO_BT))); }

// pcg_options (PCG.m:24-27 defaults); false: precd is set (the hierarchy preconditions), an argument error
static inline bool pcg_opts_rule(const ipd_pcg_opts* o, double* tol, long long* maxit) {
    *tol = 1e-11;
    *maxit = 10000;
    if (!o) return true;
    if (o->precd != -1) return false;
    if (o->retol >= 0) *tol = o->retol;
    if (o->maxit >= 0) *maxit = o->maxit;
    return true;
}

// ipd_amg_pcg_planned: the launch path, or the whole loop as one launch of k_pcg_small on a hierarchy planned for
// the single-workgroup solve (the values ipd_amg_pcg_mode reports)
enum PcgRoute { PCG_LAUNCHES = 0, PCG_ONE_LAUNCH = 1 };
static inline PcgRoute pcg_route(bool small_ok, long long maxit) {
    return (small_ok && maxit >= 0 && maxit <= PCG_SMALL_MAXIT) ? PCG_ONE_LAUNCH : PCG_LAUNCHES;
}

// slot of resk (maxit per column) that column c's residual after iteration it >= 1 goes to
static inline size_t pcg_resk_slot(long long c, long long maxit, long long it) {
    return (size_t)c * (size_t)maxit + (size_t)(it - 1);
}
// column stride of solve_multi's histories rel_resk and rhok: entry 0 and one per cycle
static inline long long multi_hist_stride(long long maxit) { return maxit + 1; }
