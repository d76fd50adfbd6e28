// AMG setup, coarsening: Ruge-Stueben strength and the C/F splittings -- mis_set, the live one, launch by launch
// and as one launch, and cf_split, the one north_star names (AMG/strength.m:6-18, mis_set.m:9-67, cf_split.m:6-16).
// Integer / compare work and strictly ordered fp64 arithmetic (no FMA contraction): strength values, masks and
// the count of random numbers consumed are BIT-IDENTICAL to the oracle's.
#pragma clang fp contract(off)

#include "ipd_setup_internal.h"

#include <cmath>
#include <cstring>

// ---------------------------------------------------------------------------
// strength                                                (AMG/strength.m:7-18)
// ---------------------------------------------------------------------------
// max_row(i) = max over the row of D-A; the diagonal of D-A is an implicit zero,
// so the maximum is never negative; "<= 0 -> Inf" (strength.m:9-10).
__global__ __launch_bounds__(256) void k_rowmax(int nr, const int* __restrict__ rp,
                                                const int* __restrict__ ci,
                                                const double* __restrict__ va,
                                                double* __restrict__ maxrow,
                                                double* __restrict__ diag) {
    WAVE_ROWS(r, nr) {
        double mx = 0.0, dg = 0.0;
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            const int j = ci[t];
            const double v = va[t];
            if (j == r)
                dg = v;
            else
                mx = fmax(mx, -v);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            mx = fmax(mx, __shfl_xor(mx, d));
            dg += __shfl_xor(dg, d);  // at most one lane holds the diagonal
        }
        if (lane == 0) {
            maxrow[r] = mx > 0.0 ? mx : INFINITY;
            diag[r] = dg;
        }
    }
}

// strong(t) = [ -a_ij / min(max_row(i), max_row(j)) >= theta ], j != i   (mis_set.m:25)
// degi = column counts of the mask (mis_set.m:28), rowcnt = row counts (mis_set.m:67)
__global__ __launch_bounds__(256) void k_strong(int nr, const int* __restrict__ rp,
                                                const int* __restrict__ ci,
                                                const double* __restrict__ va,
                                                const double* __restrict__ maxrow, double theta,
                                                uint8_t* __restrict__ strong,
                                                int* __restrict__ degi, int* __restrict__ rowcnt) {
    WAVE_ROWS(r, nr) {
        const double mr = maxrow[r];
        int cnt = 0;
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            const int j = ci[t];
            bool f = false;
            if (j != r) {
                const double sv = (-va[t]) / fmin(mr, maxrow[j]);
                f = sv >= theta;
            }
            strong[t] = f ? 1 : 0;
            if (f) {
                atomicAdd(&degi[j], 1);
                ++cnt;
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
        if (lane == 0) rowcnt[r] = cnt;
    }
}

void amg_rowmax(ipd_ctx* ctx, const Csr& A, double* maxrow, double* diag) {
    hipLaunchKernelGGL(k_rowmax, dim3(rows_grid(A.nr)), dim3(256), 0, ctx->stream, A.nr, A.rp, A.ci,
                       A.va, maxrow, diag);
    IPD_KERNEL_CHECK();
}

void amg_strength_mask(ipd_ctx* ctx, const Csr& A, double theta, uint8_t* strong, int* degi,
                       int* rowcnt) {
    Arena& tmp = *ctx->scratch;
    double* maxrow = tmp.alloc<double>((size_t)A.nr);
    double* diag = tmp.alloc<double>((size_t)A.nr);
    IPD_HIP(hipMemsetAsync(degi, 0, sizeof(int) * (size_t)std::max(A.nr, 1), ctx->stream));
    amg_rowmax(ctx, A, maxrow, diag);
    hipLaunchKernelGGL(k_strong, dim3(rows_grid(A.nr)), dim3(256), 0, ctx->stream, A.nr, A.rp, A.ci,
                       A.va, maxrow, theta, strong, degi, rowcnt);
    IPD_KERNEL_CHECK();
}

// strength VALUES for ipd_strength (zero where dropped; compacted afterwards)
__global__ __launch_bounds__(256) void k_strength_values(int nr, const int* __restrict__ rp,
                                                         const int* __restrict__ ci,
                                                         const double* __restrict__ va,
                                                         const double* __restrict__ maxrow,
                                                         int which, double* __restrict__ out) {
    WAVE_ROWS(r, nr) {
        const double mr = maxrow[r];
        for (int t = rp[r] + lane; t < rp[r + 1]; t += 64) {
            const int j = ci[t];
            double sv = 0.0;
            if (j != r) sv = (-va[t]) / (which == 1 ? mr : fmin(mr, maxrow[j]));
            out[t] = sv;
        }
    }
}

// ---------------------------------------------------------------------------
// mis_set                                                  (AMG/mis_set.m:25-67)
// ---------------------------------------------------------------------------
__global__ void k_flag_pos(int n, const int* __restrict__ v, int* __restrict__ flag) {
    THREAD_ELEMS(i, n) flag[i] = v[i] > 0 ? 1 : 0;
}

// deg(idx) = deg(idx) + 0.1*rand(sum(idx),1)  (:35);  isF(deg==0) = true (:40)
__global__ void k_deg_init(int n, const int* __restrict__ degi, const int* __restrict__ rank,
                           const double* __restrict__ randv, double* __restrict__ deg,
                           uint8_t* __restrict__ isC, uint8_t* __restrict__ isF,
                           uint8_t* __restrict__ isU, uint8_t* __restrict__ isS) {
    THREAD_ELEMS(i, n) {
        const int d = degi[i];
        double dv = 0.0;
        if (d > 0) {
            const double tie = 0.1 * randv[rank[i]];
            dv = (double)d + tie;
        }
        deg[i] = dv;
        isC[i] = 0;
        isF[i] = d == 0 ? 1 : 0;
        isU[i] = 1;
        isS[i] = d > 0 ? 1 : 0;   // isS = deg > 0 of the first round (:47)
    }
}

// edges (i,j), i<j, of triu(As(S,S),1): the smaller degree loses; ties keep the
// smaller index (:49-52).  Every write stores 0, so the races are benign.
__global__ __launch_bounds__(256) void k_mis_sel_kill(int nr, const int* __restrict__ rp,
                                                      const int* __restrict__ ci,
                                                      const uint8_t* __restrict__ strong,
                                                      const double* __restrict__ deg,
                                                      uint8_t* __restrict__ isS,
                                                      int* __restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x < 2) counts[threadIdx.x] = 0;   // summed by k_mis_settle
    WAVE_ROWS(i, nr) {
        const double di = deg[i];
        if (di > 0.0) {
            for (int t = rp[i] + lane; t < rp[i + 1]; t += 64) {
                const int j = ci[t];
                if (strong[t] && j > i) {
                    const double dj = deg[j];
                    if (dj > 0.0) {
                        if (di >= dj)
                            isS[j] = 0;
                        else
                            isS[i] = 0;
                    }
                }
            }
        }
    }
}

// The rest of a round in one launch, one wave per node (:53-59 and the loop test :42):
//   isC(isS) = true;  [i,~] = find(As(:,isC)); isF(i) = true;  isU = ~(isF|isC);  deg(~isU) = 0
// A neighbour is in C after this round iff it was before or survived the selection, and both
// flags are final when this kernel starts, so no node waits for another one's commit.  The
// selection of the next round, isS = deg > 0 = isU, goes to a second buffer because isS is still
// being read here.
__global__ __launch_bounds__(256) void k_mis_settle(int nr, const int* __restrict__ rp,
                                                    const int* __restrict__ ci,
                                                    const uint8_t* __restrict__ strong,
                                                    const uint8_t* __restrict__ isS,
                                                    uint8_t* __restrict__ isC,
                                                    uint8_t* __restrict__ isF,
                                                    uint8_t* __restrict__ isU,
                                                    double* __restrict__ deg,
                                                    uint8_t* __restrict__ isS_next,
                                                    int* __restrict__ counts) {
    int nc = 0, nu = 0;
    WAVE_ROWS(i, nr) {
        bool hit = false;
        for (int t = rp[i] + lane; t < rp[i + 1]; t += 64) {
            const int j = ci[t];
            if (strong[t] && (isC[j] || isS[j])) hit = true;
        }
        hit = __any(hit);
        if (lane == 0) {
            const bool c = isC[i] || isS[i];
            const bool f = isF[i] || hit;
            const bool u = !(c || f);
            if (c) isC[i] = 1;
            if (f) isF[i] = 1;
            isU[i] = u ? 1 : 0;
            isS_next[i] = u ? 1 : 0;
            if (!u) deg[i] = 0.0;
            nc += c;
            nu += u;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (nc) atomicAdd(&counts[0], nc);
        if (nu) atomicAdd(&counts[1], nu);
    }
}

__global__ void k_mis_absorb(int n, uint8_t* __restrict__ isU, uint8_t* __restrict__ isC) {
    THREAD_ELEMS(i, n) if (isU[i]) {
        isC[i] = 1;
        isU[i] = 0;
    }
}

// iso = sum(As,2)==0; isC(iso) = true; isF(iso) = false   (:67)
__global__ void k_mis_iso(int n, const int* __restrict__ rowcnt, uint8_t* __restrict__ isC,
                          uint8_t* __restrict__ isF) {
    THREAD_ELEMS(i, n) if (rowcnt[i] == 0) {
        isC[i] = 1;
        isF[i] = 0;
    }
}


// ---------------------------------------------------------------------------
// mis_set of a SMALL level in one launch                   (AMG/mis_set.m:25-67)
// ---------------------------------------------------------------------------
// Levels >= 2 of the drivers' Newton systems have a few hundred rows and a few thousand entries.
// There the launch-per-step form above is ~20 launches and 4 host round trips per level (strength,
// degree flags + scan, random numbers, every round of the selection, the clean-up, the C index
// scan): 100-150 us of launch and round-trip latency around ~10 us of work.  For levels of at most
// 1024 rows and MIS_SMALL_NNZ entries ONE workgroup does all of it, thread i = node i: the rows'
// strong neighbours are listed once in LDS (16-bit indices), the rounds run on those lists with the
// degrees and flags in LDS, and the loop test of mis_set.m:42 is taken on the device.  The random
// numbers of mis_set.m:35 are handed in as the NEXT N numbers of the stream; the kernel uses the
// first `nconn` of them (as the reference does) and reports nconn, and the host then consumes exactly
// that many (ipd_rng state saved and restored around the peek).  Same statements, same order of
// evaluation per entry as k_rowmax / k_strong / k_deg_init / k_mis_sel_kill / k_mis_settle /
// k_mis_absorb / k_mis_iso / k_u8_to_flag / k_count_bad_split + the scans: identical bits.
struct MisSmallArgs {
    int N, N0;
    const int* rp;
    const int* ci;
    const double* va;
    double theta;
    const double* randv;      // N values: the stream's next numbers
    uint8_t* strong;          // out: nnz flags
    double* maxrow;           // out (interpolation needs them again, transfer.m:49-51)
    double* diag;
    uint8_t* isC;             // out
    uint8_t* isF;             // out
    int* cidx;                // out: N + 1 entries, cidx[N] = Nc
    volatile unsigned* box;   // mailbox: {status, nconn, Nc, bad, rounds}; status 1 = degenerate branch (:30-34)
    unsigned ticket;
};
__device__ __forceinline__ int mis_block_exscan(int v, int* wsum, int* total) {   // 1024 threads
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int sgm = wsum[k];
        if (k < w) woff += sgm;
        tot += sgm;
    }
    *total = tot;
    return woff + x - v;
}
__global__ __launch_bounds__(1024) void k_mis_small(const MisSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) char mis_raw[];
    __shared__ int wsum[16];
    __shared__ int s_cnt[2];
    const int N = a.N;
    // L lanes per node (the largest of 1, 2, 4, 8 with N L <= 1024): a row's entries -- in memory for the
    // strength pass, its strong-neighbour list in LDS for the rounds -- are strided over the group, so a
    // hub row of 60-300 entries is a few trips, not a chain of as many; lane 0 of the group owns the node
    int L = 1;
    while (L < 8 && N * (L * 2) <= 1024) L <<= 1;
    const int i = threadIdx.x / L, sub = threadIdx.x % L;
    const bool valid = i < N, owner = valid && sub == 0;
    double* maxrow = reinterpret_cast<double*>(mis_raw);            // N
    double* deg = maxrow + MIS_SMALL_ROWS;                          // N
    int* degi = reinterpret_cast<int*>(deg + MIS_SMALL_ROWS);       // N
    int* scnt = degi + MIS_SMALL_ROWS;                              // N: strong neighbours listed so far
    uint8_t* fC = reinterpret_cast<uint8_t*>(scnt + MIS_SMALL_ROWS);
    uint8_t* fF = fC + MIS_SMALL_ROWS;
    uint8_t* fU = fF + MIS_SMALL_ROWS;
    uint8_t* fS = fU + MIS_SMALL_ROWS;
    uint8_t* fS2 = fS + MIS_SMALL_ROWS;
    unsigned short* sci = reinterpret_cast<unsigned short*>(fS2 + MIS_SMALL_ROWS);   // strong neighbours, row i at [r0, ..)
    const int r0 = valid ? a.rp[i] : 0, r1 = valid ? a.rp[i + 1] : 0;
    auto group_or = [&](bool v) {
        int x = v ? 1 : 0;
        for (int d = 1; d < L; d <<= 1) x |= __shfl_xor(x, d);
        return x != 0;
    };
    // ---- strength.m:7-10 (k_rowmax); eight entries per lane and trip, all loads of a trip in flight
    {
        double mx = 0.0, dg = 0.0;
        for (int t0 = r0 + sub; t0 < r1; t0 += 8 * L) {
            int jj[8];
            double vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = t0 + u * L < r1 ? t0 + u * L : r0;
                jj[u] = a.ci[t];
                vv[u] = a.va[t];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (t0 + u * L < r1) {
                    if (jj[u] == i)
                        dg = vv[u];
                    else
                        mx = fmax(mx, -vv[u]);
                }
            }
        }
        for (int d = 1; d < L; d <<= 1) {
            mx = fmax(mx, __shfl_xor(mx, d));
            dg += __shfl_xor(dg, d);   // at most one lane holds the diagonal
        }
        if (owner) {
            const double m = mx > 0.0 ? mx : INFINITY;
            maxrow[i] = m;
            a.maxrow[i] = m;
            a.diag[i] = dg;
            degi[i] = 0;
            scnt[i] = 0;
        }
    }
    __syncthreads();
    // ---- mis_set.m:25-29 (k_strong): the mask, its column counts (deg) and row counts; the strong
    // neighbours of row i are listed at sci[r0 ..) in any order (the rounds only ask whether ANY / EVERY
    // neighbour has a property, so the order of the list does not matter)
    {
        const double mr = valid ? maxrow[i] : 1.0;
        for (int t0 = r0 + sub; t0 < r1; t0 += 8 * L) {
            int jj[8];
            double vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = t0 + u * L < r1 ? t0 + u * L : r0;
                jj[u] = a.ci[t];
                vv[u] = a.va[t];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (t0 + u * L < r1) {
                    const int j = jj[u];
                    bool f = false;
                    if (j != i) {
                        const double sv = (-vv[u]) / fmin(mr, maxrow[j]);
                        f = sv >= a.theta;
                    }
                    a.strong[t0 + u * L] = f ? 1 : 0;
                    if (f) {
                        atomicAdd(&degi[j], 1);
                        sci[r0 + atomicAdd(&scnt[i], 1)] = (unsigned short)j;
                    }
                }
            }
        }
    }
    __syncthreads();   // degi, scnt and the lists are final
    const int rowcnt = valid ? scnt[i] : 0;
    const int d = valid ? degi[i] : 0;
    int nconn = 0;
    const int rank = mis_block_exscan((owner && d > 0) ? 1 : 0, wsum, &nconn);
    if ((double)nconn < 0.25 * sqrt((double)N)) {              // :30-34: the host takes this (rare) branch
        if (threadIdx.x == 0) {
            a.box[16] = 1u;
            a.box[17] = (unsigned)nconn;
            __threadfence_system();
            a.box[0] = a.ticket;
        }
        return;
    }
    // ---- :35-40 (k_deg_init)
    if (owner) {
        double dv = 0.0;
        if (d > 0) {
            const double tie = 0.1 * a.randv[rank];
            dv = (double)d + tie;
        }
        deg[i] = dv;
        fC[i] = 0;
        fF[i] = d == 0 ? 1 : 0;
        fU[i] = 1;
        fS[i] = d > 0 ? 1 : 0;
    }
    __syncthreads();
    // ---- :42-65: the rounds
    const int s0 = r0, s1 = r0 + rowcnt;
    int sumC = 0, sumU = N, rounds = 0;
    uint8_t* cur = fS;
    uint8_t* nxt = fS2;
    while ((double)sumC < (double)N / 2.0 && sumU > a.N0 && rounds <= N + 8) {
        ++rounds;
        if (valid) {                                           // k_mis_sel_kill (:49-52)
            const double di = deg[i];
            if (di > 0.0)
                for (int t = s0 + sub; t < s1; t += L) {
                    const int j = sci[t];
                    if (j > i) {
                        const double dj = deg[j];
                        if (dj > 0.0) {
                            if (di >= dj)
                                cur[j] = 0;
                            else
                                cur[i] = 0;
                        }
                    }
                }
        }
        if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        bool hit = false;                                      // k_mis_settle (:53-59)
        if (valid)
            for (int t = s0 + sub; t < s1; t += L) {
                const int j = sci[t];
                if (fC[j] || cur[j]) hit = true;
            }
        hit = group_or(hit);
        int c1 = 0, u1 = 0;
        if (owner) {
            const bool c = fC[i] || cur[i];
            const bool f = fF[i] || hit;
            const bool u = !(c || f);
            c1 = c ? 1 : 0;
            u1 = u ? 1 : 0;
            nxt[i] = u ? 1 : 0;
            fU[i] = u ? 1 : 0;
            if (f) fF[i] = 1;
            if (!u) deg[i] = 0.0;
        }
        // (fC is read by the neighbours in this phase: committed after the barrier below)
        const unsigned long long bc = __ballot(c1 != 0), bu = __ballot(u1 != 0);
        if ((threadIdx.x & 63) == 0) {
            if (bc) atomicAdd(&s_cnt[0], __popcll(bc));
            if (bu) atomicAdd(&s_cnt[1], __popcll(bu));
        }
        __syncthreads();
        if (owner && c1) fC[i] = 1;
        sumC = s_cnt[0];
        sumU = s_cnt[1];
        uint8_t* tsw = cur;
        cur = nxt;
        nxt = tsw;
        __syncthreads();
        if (sumU <= a.N0) {                                    // :61-64 (k_mis_absorb)
            if (owner && fU[i]) {
                fC[i] = 1;
                fU[i] = 0;
            }
            sumU = 0;
            __syncthreads();
        }
    }
    // ---- :67 (k_mis_iso), then the C index scan and the consistency count of transfer.m:46-47
    int isc = 0, isf = 0;
    if (owner) {
        isc = fC[i];
        isf = fF[i];
        if (rowcnt == 0) {
            isc = 1;
            isf = 0;
        }
        a.isC[i] = (uint8_t)isc;
        a.isF[i] = (uint8_t)isf;
    }
    int Nc = 0, bad = 0;
    const int cpos = mis_block_exscan(owner ? isc : 0, wsum, &Nc);
    mis_block_exscan((owner && (isc != 0) == (isf != 0)) ? 1 : 0, wsum, &bad);
    if (owner) a.cidx[i] = cpos;
    if (threadIdx.x == 0) {
        a.cidx[N] = Nc;
        a.box[16] = 0u;
        a.box[17] = (unsigned)nconn;
        a.box[18] = (unsigned)Nc;
        a.box[19] = (unsigned)bad;
        a.box[20] = (unsigned)rounds;
        __threadfence_system();
        a.box[0] = a.ticket;
    }
}

// A level plan_mis_small admits.  -> true: done (Nc, bad filled, cidx / maxrow / diag written); false: not taken
// (mailbox off) or the degenerate branch of :30-34 came up, and the caller runs the launch-per-step form
static bool mis_set_small(ipd_ctx* ctx, const Csr& A, double theta, ipd_rng* rng, uint8_t* isC, uint8_t* isF,
                          uint8_t* strong, double* maxrow, double* diag, int* cidx, int* Nc, int* bad) {
    const int N = A.nr;
    unsigned ticket = 0;
    if (!ctx->mailbox_begin(&ticket)) return false;
    Arena& tmp = *ctx->scratch;
    // peek at the stream's next N numbers (state restored below; a replay stream may hold fewer)
    std::vector<double> rv((size_t)N, 0.0);
    {
        const bool rp = rng->replay;
        const int64_t have = rp ? std::max<int64_t>(0, (int64_t)rng->values.size() - rng->consumed) : N;
        const int64_t take = std::min<int64_t>(N, have);
        uint32_t mt[624];
        std::memcpy(mt, rng->mt, sizeof(mt));
        const int mti = rng->mti;
        const int64_t consumed = rng->consumed;
        if (take > 0) rng->fill(rv.data(), take);
        std::memcpy(rng->mt, mt, sizeof(mt));
        rng->mti = mti;
        rng->consumed = consumed;
    }
    double* drand = tmp.alloc<double>((size_t)N);
    ctx->upload(drand, rv.data(), (size_t)N);
    MisSmallArgs a;
    a.N = N;
    a.N0 = std::min((int)std::floor(std::sqrt((double)N)) + 1, 25);   // :12
    a.rp = A.rp;
    a.ci = A.ci;
    a.va = A.va;
    a.theta = theta;
    a.randv = drand;
    a.strong = strong;
    a.maxrow = maxrow;
    a.diag = diag;
    a.isC = isC;
    a.isF = isF;
    a.cidx = cidx;
    a.box = ctx->mailbox;
    a.ticket = ticket;
    const size_t lds = 16 * (size_t)MIS_SMALL_ROWS + 8 * (size_t)MIS_SMALL_ROWS + 5 * (size_t)MIS_SMALL_ROWS +
                       2 * (size_t)std::max(A.nnz, 1) + 64;
    IPD_OPTIN_LDS(ctx, k_mis_small, 156 * 1024);
    hipLaunchKernelGGL(k_mis_small, dim3(1), dim3(1024), lds, ctx->stream, a);
    IPD_KERNEL_CHECK();
    unsigned w[5] = {0, 0, 0, 0, 0};
    ctx->mailbox_wait(ticket, w, sizeof(w));
    if (w[0] != 0) return false;                     // degenerate branch: nothing consumed yet
    IPD_REQUIRE((int)w[4] <= N + 8, IPD_E_NUMERIC, "mis_set: no progress");
    std::vector<double> used((size_t)w[1]);
    rng->fill(used.data(), (int64_t)w[1]);           // mis_set.m:35 consumes sum(deg > 0) numbers
    *Nc = (int)w[2];
    *bad = (int)w[3];
    return true;
}

void amg_mis_set(ipd_ctx* ctx, const Csr& A, double theta, ipd_rng* rng, uint8_t* isC,
                 uint8_t* isF, uint8_t* strong_out) {
    IPD_REQUIRE(rng, IPD_E_ARG, "mis_set needs a rand stream");
    IPD_REQUIRE(theta > 0, IPD_E_ARG, "mis_set: theta must be positive");
    const int N = A.nr;
    Arena& tmp = *ctx->scratch;
    uint8_t* strong = strong_out ? strong_out : tmp.alloc<uint8_t>((size_t)A.nnz);
    int* degi = tmp.alloc<int>((size_t)N + 1);
    int* rowcnt = tmp.alloc<int>((size_t)N + 1);
    int* flag = tmp.alloc<int>((size_t)N + 1);
    int* rank = tmp.alloc<int>((size_t)N + 2);
    double* deg = tmp.alloc<double>((size_t)N);
    uint8_t* isU = tmp.alloc<uint8_t>((size_t)N);
    uint8_t* isS = tmp.alloc<uint8_t>((size_t)N);
    int* counts = tmp.alloc<int>(2);
    const int N0 = std::min((int)std::floor(std::sqrt((double)N)) + 1, 25);  // :12
    amg_strength_mask(ctx, A, theta, strong, degi, rowcnt);                  // :25-29
    const int g = elems_grid(N);
    hipLaunchKernelGGL(k_flag_pos, dim3(g), dim3(256), 0, ctx->stream, N, degi, flag);
    IPD_KERNEL_CHECK();
    const int nconn = exclusive_scan_total(ctx, flag, rank, N);
    if ((double)nconn < 0.25 * std::sqrt((double)N)) {                       // :30-34
        std::vector<double> rv((size_t)N0);
        rng->fill(rv.data(), N0);
        std::vector<uint8_t> hc((size_t)N, 0), hf((size_t)N, 1);
        for (int k = 0; k < N0; ++k) {
            long long pick = (long long)std::ceil(rv[k] * (double)N) - 1;
            if (pick < 0) pick = 0;  // rand never returns exactly 0; guard anyway
            if (pick >= N) pick = N - 1;
            hc[(size_t)pick] = 1;
            hf[(size_t)pick] = 0;
        }
        ctx->upload(isC, hc.data(), (size_t)N);
        ctx->upload(isF, hf.data(), (size_t)N);
        return;
    }
    std::vector<double> rv((size_t)nconn);
    rng->fill(rv.data(), nconn);                                             // :35
    double* drand = tmp.alloc<double>((size_t)nconn);
    ctx->upload(drand, rv.data(), (size_t)nconn);
    uint8_t* isS2 = tmp.alloc<uint8_t>((size_t)N);
    hipLaunchKernelGGL(k_deg_init, dim3(g), dim3(256), 0, ctx->stream, N, degi, rank, drand, deg,
                       isC, isF, isU, isS);
    IPD_KERNEL_CHECK();
    int sumC = 0, sumU = N;
    int rounds = 0;
    while ((double)sumC < (double)N / 2.0 && sumU > N0) {                    // :42
        IPD_REQUIRE(++rounds <= N + 8, IPD_E_NUMERIC, "mis_set: no progress");
        // two launches per round: the edge-wise selection, then everything that follows it
        hipLaunchKernelGGL(k_mis_sel_kill, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, A.rp,
                           A.ci, strong, deg, isS, counts);
        hipLaunchKernelGGL(k_mis_settle, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, A.rp, A.ci,
                           strong, isS, isC, isF, isU, deg, isS2, counts);
        IPD_KERNEL_CHECK();
        std::swap(isS, isS2);
        int hc[2];
        ctx->fetch(counts, hc, 2);
        sumC = hc[0];
        sumU = hc[1];
        if (sumU <= N0) {                                                    // :61-64
            hipLaunchKernelGGL(k_mis_absorb, dim3(g), dim3(256), 0, ctx->stream, N, isU, isC);
            IPD_KERNEL_CHECK();
            sumU = 0;
        }
    }
    hipLaunchKernelGGL(k_mis_iso, dim3(g), dim3(256), 0, ctx->stream, N, rowcnt, isC, isF);
    IPD_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// cf_split                                                (AMG/cf_split.m:6-16)
// ---------------------------------------------------------------------------
// The sequential greedy pass (k = 1..N: an unvisited k becomes C and its
// neighbours F) yields the lexicographically-first maximal independent set:
// k is C iff no lower-indexed neighbour is C.  Parallel form, one workgroup:
// an undecided node becomes F as soon as a lower neighbour is C, and C as soon
// as every lower neighbour is F.  Decisions are final, so in-place updates and
// any interleaving give the identical (bit-exact) result.
__global__ __launch_bounds__(1024) void k_cf_split(int n, const int* __restrict__ rp,
                                                   const int* __restrict__ ci,
                                                   uint8_t* __restrict__ state /*0 U,1 C,2 F*/,
                                                   int* __restrict__ rounds_out) {
    __shared__ int pending;
    int rounds = 0;
    while (true) {
        if (threadIdx.x == 0) pending = 0;
        __syncthreads();
        bool mine = false;
        for (int k = threadIdx.x; k < n; k += 1024) {
            if (state[k] != 0) continue;
            bool anyC = false, anyU = false;
            for (int t = rp[k]; t < rp[k + 1]; ++t) {
                const int j = ci[t];
                if (j >= k) break;  // columns ascend: only lower neighbours matter
                const uint8_t sj = state[j];
                anyC |= (sj == 1);
                anyU |= (sj == 0);
            }
            if (anyC)
                state[k] = 2;
            else if (!anyU)
                state[k] = 1;
            else
                mine = true;
        }
        if (mine) pending = 1;
        __syncthreads();
        ++rounds;
        const int p = pending;
        __syncthreads();
        if (!p || rounds > n + 2) break;  // every round decides >= 1 node; the bound is a hang guard
    }
    if (threadIdx.x == 0) *rounds_out = rounds;
}

__global__ void k_state_to_masks(int n, const uint8_t* __restrict__ state,
                                 uint8_t* __restrict__ isC, uint8_t* __restrict__ isF) {
    THREAD_ELEMS(i, n) {
        isC[i] = state[i] == 1;
        isF[i] = state[i] == 2;
    }
}

static void amg_cf_split(ipd_ctx* ctx, const Csr& S, uint8_t* isC, uint8_t* isF) {
    Arena& tmp = *ctx->scratch;
    uint8_t* state = tmp.alloc<uint8_t>((size_t)S.nr);
    int* rounds = tmp.alloc<int>(1);
    IPD_HIP(hipMemsetAsync(state, 0, (size_t)std::max(S.nr, 1), ctx->stream));
    hipLaunchKernelGGL(k_cf_split, dim3(1), dim3(1024), 0, ctx->stream, S.nr, S.rp, S.ci, state,
                       rounds);
    IPD_KERNEL_CHECK();
    hipLaunchKernelGGL(k_state_to_masks, dim3(elems_grid(S.nr)), dim3(256), 0, ctx->stream, S.nr,
                       state, isC, isF);
    IPD_KERNEL_CHECK();
}

// ---------------------------------------------------------------------------
// a level's split for amg_transfer                        (AMG/transfer.m:41-47)
// ---------------------------------------------------------------------------
__global__ void k_u8_to_flag(int n, const uint8_t* __restrict__ a, int* __restrict__ f) {
    THREAD_ELEMS(i, n) f[i] = a[i] ? 1 : 0;
}
__global__ void k_count_bad_split(int n, const uint8_t* __restrict__ isC,
                                  const uint8_t* __restrict__ isF, int* __restrict__ bad) {
    THREAD_ELEMS(i, n) if ((isC[i] != 0) == (isF[i] != 0)) atomicAdd(bad, 1);
}

void amg_mask_index(ipd_ctx* ctx, const uint8_t* mask, int* flag, int* idx, int N) {
    hipLaunchKernelGGL(k_u8_to_flag, dim3(elems_grid(N)), dim3(256), 0, ctx->stream, N, mask, flag);
    IPD_KERNEL_CHECK();
    exclusive_scan_i32(ctx, flag, idx, N);
}

void amg_level_split(ipd_ctx* ctx, const Csr& A, double theta, ipd_rng* rng, bool try_small, LevelSplit* s) {
    const int N = A.nr;
    int meta[2] = {0, 0};
    s->small_done = try_small && mis_set_small(ctx, A, theta, rng, s->isC, s->isF, s->strong, s->maxrow, s->diag,
                                               s->cidx, &meta[0], &meta[1]);
    if (!s->small_done) {
        amg_mis_set(ctx, A, theta, rng, s->isC, s->isF, s->strong);          // transfer.m:41
        int* flag = ctx->scratch->alloc<int>((size_t)N + 1);
        IPD_HIP(hipMemsetAsync(s->cidx + N + 1, 0, sizeof(int), ctx->stream));
        hipLaunchKernelGGL(k_u8_to_flag, dim3(elems_grid(N)), dim3(256), 0, ctx->stream, N, s->isC, flag);
        hipLaunchKernelGGL(k_count_bad_split, dim3(elems_grid(N)), dim3(256), 0, ctx->stream, N, s->isC,
                           s->isF, s->cidx + N + 1);
        IPD_KERNEL_CHECK();
        exclusive_scan_i32(ctx, flag, s->cidx, N);
        ctx->fetch(s->cidx + N, meta, 2);
    }
    s->Nc = meta[0];
    s->bad = meta[1];
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_strength(ipd_ctx* ctx, const ipd_csc* A, int which, ipd_csc_out* S) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && A && S, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(which == 1 || which == 2, IPD_E_ARG, "strength: which must be 1 or 2");
        CallScope scope(ctx);
        Arena& tmp = *ctx->scratch;
        Csr a;
        csr_upload_from_csc(ctx, tmp, A, false, &a);
        double* maxrow = tmp.alloc<double>((size_t)a.nr);
        double* diag = tmp.alloc<double>((size_t)a.nr);
        Csr v = a;
        v.va = tmp.alloc<double>((size_t)a.nnz);
        hipLaunchKernelGGL(k_rowmax, dim3(rows_grid(a.nr)), dim3(256), 0, ctx->stream, a.nr, a.rp,
                           a.ci, a.va, maxrow, diag);
        hipLaunchKernelGGL(k_strength_values, dim3(rows_grid(a.nr)), dim3(256), 0, ctx->stream, a.nr,
                           a.rp, a.ci, a.va, maxrow, which, v.va);
        IPD_KERNEL_CHECK();
        Csr clean;
        csr_drop_zeros(ctx, tmp, v, &clean);
        csr_download_as_csc(ctx, clean, false, S);
    });
}

extern "C" int ipd_cf_split(ipd_ctx* ctx, const ipd_csc* S, uint8_t* indC, uint8_t* indF) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && S && indC && indF, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(S->nrows == S->ncols, IPD_E_ARG, "cf_split: S must be square");
        CallScope scope(ctx);
        Arena& tmp = *ctx->scratch;
        Csr s;
        csr_upload_from_csc(ctx, tmp, S, true, &s);  // graph(S) requires a symmetric S
        uint8_t* dC = tmp.alloc<uint8_t>((size_t)s.nr);
        uint8_t* dF = tmp.alloc<uint8_t>((size_t)s.nr);
        amg_cf_split(ctx, s, dC, dF);
        ctx->fetch(dC, indC, (size_t)s.nr);
        ctx->fetch(dF, indF, (size_t)s.nr);
    });
}

// strong flags (aligned with A's pattern) -> CSR pattern matrix with values 1
__global__ void k_flag_to_value(int nnz, const uint8_t* __restrict__ f, double* __restrict__ v) {
    THREAD_ELEMS(i, nnz) v[i] = f[i] ? 1.0 : 0.0;
}

extern "C" int ipd_mis_set(ipd_ctx* ctx, const ipd_csc* A, double theta, ipd_rng* rng,
                           uint8_t* isC, uint8_t* isF, ipd_csc_out* As) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && A && rng && isC && isF, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(A->nrows == A->ncols, IPD_E_ARG, "mis_set: A must be square");
        CallScope scope(ctx);
        Arena& tmp = *ctx->scratch;
        Csr a;
        csr_upload_from_csc(ctx, tmp, A, false, &a);
        uint8_t* dC = tmp.alloc<uint8_t>((size_t)a.nr);
        uint8_t* dF = tmp.alloc<uint8_t>((size_t)a.nr);
        uint8_t* strong = tmp.alloc<uint8_t>((size_t)std::max(a.nnz, 1));
        amg_mis_set(ctx, a, theta, rng, dC, dF, strong);
        ctx->fetch(dC, isC, (size_t)a.nr);
        ctx->fetch(dF, isF, (size_t)a.nr);
        if (As) {
            Csr v = a;
            v.va = tmp.alloc<double>((size_t)std::max(a.nnz, 1));
            hipLaunchKernelGGL(k_flag_to_value, dim3(elems_grid(a.nnz)), dim3(256), 0, ctx->stream,
                               a.nnz, strong, v.va);
            IPD_KERNEL_CHECK();
            Csr clean;
            csr_drop_zeros(ctx, tmp, v, &clean);
            csr_download_as_csc(ctx, clean, false, As);
        }
    });
}
