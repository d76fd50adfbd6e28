// The block form of the launch-path cycle (ipd_block.hip): the N x W work blocks of a hierarchy and the host
// functions through which another unit (ipd_block_krylov.hip) runs the block cycle and the layout change at a
// call's edges.  A kernel is launched only by the unit that defines it.  Host-only.  The host decisions are in
// ipd_krylov_plan.h (host-clean).
#pragma once

#include "ipd_amg_internal.h"
#include "ipd_krylov_plan.h"

struct BlockVecs {   // a level's N x W work blocks
    double* r = nullptr;
    double* e = nullptr;
    double* e2 = nullptr;
    double* w = nullptr;
    double* rr = nullptr;
    bool e_zero = true;
};

struct BlockState {
    int W = 0;                      // width the blocks were made for
    std::vector<BlockLevel> lv;     // 1-based
    std::vector<BlockVecs> v;       // 1-based
    double* x[2] = {nullptr, nullptr};
    double* b = nullptr;
    double* hist = nullptr;         // HB x W
    double* pcg_work = nullptr;     // 4 N_J x W
};

// ---- ipd_block.hip ----
// the hierarchy's blocks, (re)made when W is wider than what they were made for
BlockState* block_state(ipd_amg* h, int W);
// v[1].e = one cycle from zero on v[1].r, W columns wide (W in {1, 2, 4, 8}); wc: W cycle
void block_cycle(ipd_amg* h, BlockState* bs, int W, bool wc);
// column-major (leading dimension ld, ncol columns; src NULL: zeros) -> N x W interleaved, missing columns zero
void block_in(ipd_ctx* ctx, int N, int W, int ncol, const double* src, long long ld, double* dst);
// N x W interleaved -> the first ncol columns of a column-major block
void block_out(ipd_ctx* ctx, int N, int W, int ncol, const double* src, double* dst, long long ld);

// The host-pointer form of a multi-right-hand-side entry: B and the guess go up, dev(dB, dguess, dX) runs, X comes
// back.  Rows N..ld-1 of X are the caller's: they are carried through.
template <class F>
static void block_host_call(ipd_amg* h, const double* B, long long ld, long long nrhs, const double* guess,
                            double* X, F&& dev) {
    ipd_ctx* ctx = h->ctx;
    const size_t n = (size_t)ld * (size_t)nrhs;
    double* dB = ctx->scratch->alloc<double>(n);
    double* dX = ctx->scratch->alloc<double>(n);
    double* dg = nullptr;
    ctx->upload(dB, B, n);
    if (guess) {
        dg = ctx->scratch->alloc<double>(n);
        ctx->upload(dg, guess, n);
    }
    if (ld > (long long)h->L[1].A.nr) ctx->upload(dX, X, n);
    dev(dB, dg, dX);
    ctx->fetch(dX, X, n);
}
