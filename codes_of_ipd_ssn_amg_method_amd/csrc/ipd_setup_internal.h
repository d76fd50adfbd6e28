// The setup's units and the host functions they call each other through (a kernel is launched only by the unit
// that defines it):
//   ipd_coarsen.hip   strength, mis_set in both forms, cf_split; ipd_strength, ipd_cf_split, ipd_mis_set
//   ipd_prolong.hip   the interpolation builds: P of a level from its TransferPlan
//   ipd_setup.hip     amg_transfer (plan, split, P, transpose, Galerkin products), amg_setup, the hierarchy ABI
// Every decision they carry out is ipd_setup_plan.h's.
#pragma once

#include "ipd_amg_internal.h"
#include "ipd_setup_plan.h"

#define WAVE_ROWS(r, nr)                                                    \
    const int lane = threadIdx.x & 63;                                      \
    const int wave__ = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;        \
    const int nwaves__ = (gridDim.x * blockDim.x) >> 6;                     \
    for (int r = wave__; r < (nr); r += nwaves__)

#define THREAD_ELEMS(i, n)                                                  \
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < (n);            \
         i += gridDim.x * blockDim.x)

// The C/F split of a non-bigraph level and what the interpolation reads of it, all N-sized device arrays of the
// caller: cidx has N + 2 entries (the exclusive scan of isC, cidx[N] = Nc, then a scratch word)
struct LevelSplit {
    uint8_t* isC = nullptr;
    uint8_t* isF = nullptr;
    uint8_t* strong = nullptr;   // nnz flags aligned with A's pattern
    int* cidx = nullptr;
    double* maxrow = nullptr;
    double* diag = nullptr;
    int Nc = 0, bad = 0;         // coarse nodes; nodes in neither or both sets (transfer.m:46-47)
    bool small_done = false;     // k_mis_small did it, maxrow and diag included
};

// ipd_coarsen.hip
// mis_set(A, theta) into s: as one launch where `try_small` (plan_mis_small) holds and a mailbox ticket is
// granted, else -- or when the degenerate branch of mis_set.m:30-34 comes up -- launch by launch
void amg_level_split(ipd_ctx* ctx, const Csr& A, double theta, ipd_rng* rng, bool try_small, LevelSplit* s);
void amg_rowmax(ipd_ctx* ctx, const Csr& A, double* maxrow, double* diag);          // strength.m:7-10
// idx = exclusive scan of (mask != 0), idx[N] the count; flag: N + 1 ints of scratch
void amg_mask_index(ipd_ctx* ctx, const uint8_t* mask, int* flag, int* idx, int N);

// ipd_prolong.hip: P (N x Nc, arrays out of dst, P->nnz the plan's bound while the count is lazy) in the form
// and with the row-count mode of the plan.  counts: the level's six lazy words (entries of P, P'A, Ac, the
// "Aff is not diagonal" flag, longest row of P'A), nullptr unless plan.lazy.
void amg_prolong_bigraph(ipd_ctx* ctx, Arena& dst, const Csr& A, const AmgOpts& o, const TransferPlan& plan,
                         int* counts, uint8_t* cmask, Csr* P);
void amg_prolong_classical(ipd_ctx* ctx, Arena& dst, const Csr& A, const AmgOpts& o, const TransferPlan& plan,
                           const LevelSplit& s, int* counts, Csr* P);
