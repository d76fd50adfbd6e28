// AMG setup, interpolation: P of a level in the form its TransferPlan names (AMG/transfer.m:19-63) -- level 1
// of a bigraph, the ideal interpolation, and the classical rows W1 + 0.5*W2 as one kernel per row (a wave, or a
// workgroup with a barrier per neighbour) or as an ordered product.  Strictly ordered fp64 arithmetic (no FMA
// contraction, sequential accumulation in ascending index): every form gives Pro BIT-IDENTICAL to the oracle's.
// The kernels are latency-bound at realistic sizes (N <= 4096, nnz 1e3..1e6): the design goal is few launches
// and no float atomics, not bandwidth.
#pragma clang fp contract(off)

#include "ipd_setup_internal.h"

#include <cmath>

// ---------------------------------------------------------------------------
// interpolation                                          (AMG/transfer.m:19-63)
// ---------------------------------------------------------------------------
// level 1 of a bigraph: F = first nf rows, W = (-Aff)\Afc with Aff diagonal
// (transfer.m:20-25); one lane per row, sequential, so the row sum used by the
// isnsp normalisation (:22-24) is accumulated in ascending column order.
__global__ __launch_bounds__(256) void k_bigph_count(int N, int nf, const int* __restrict__ rp,
                                                     const int* __restrict__ ci, int* rowlen,
                                                     const ScanTail st, int* __restrict__ badp) {
    // st.out != NULL: biased counts with the flag in bit 30, scanned and posted by the launch's tail;
    // otherwise plain counts (k_bigph_fill scans them) and the flag at *badp
    WAVE_ROWS(i, N) {
        if (i >= nf) {
            if (lane == 0) {
                if (st.out)
                    scan_put(rowlen, i, 1);
                else
                    rowlen[i] = 1;
            }
            continue;
        }
        int c = 0;
        bool bad = false;   // Aff is not diagonal
        for (int t = rp[i] + lane; t < rp[i + 1]; t += 64) {
            const int j = ci[t];
            if (j >= nf)
                ++c;
            else if (j != i)
                bad = true;
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
        bad = __any(bad);
        if (lane == 0) {
            if (st.out)
                scan_put(rowlen, i, c, bad);
            else {
                rowlen[i] = c;
                if (bad) *badp = 1;
            }
        }
    }
    scan_tail(st);   // P's row pointers; total and flag to the host
}

// One wave per row.  Lanes write the entries in parallel; the row sum of the isnsp
// normalisation is accumulated by lane 0 alone, sequentially in ascending column order
// (recomputing the quotients it sums, so it does not depend on the other lanes' stores).
__global__ __launch_bounds__(256) void k_bigph_fill(int N, int nf, int isnsp,
                                                    const int* __restrict__ rp,
                                                    const int* __restrict__ ci,
                                                    const double* __restrict__ va,
                                                    const int* prp,
                                                    int* __restrict__ pci, double* __restrict__ pva,
                                                    uint8_t* __restrict__ cmask,
                                                    const int* __restrict__ head_cnt, int* head_rp,
                                                    int* head_total) {
    __shared__ ScanHeadLds L;   // head_cnt != NULL: plain counts, scanned here (scan_head; N <= SCAN_HEAD_MAX)
    if (head_cnt) {
        scan_head(head_cnt, N, head_rp, head_total, L);
        prp = L.rp;
    }
    WAVE_ROWS(i, N) {
        const int pos0 = prp[i];
        if (i >= nf) {
            if (lane == 0) {
                pci[pos0] = i - nf;
                pva[pos0] = 1.0;
                cmask[i] = 1;
            }
            continue;
        }
        const int b = rp[i], e = rp[i + 1];
        // the diagonal, and the first entry of the C block (columns ascend: a suffix)
        double dii = 0.0;
        int first = e;
        for (int t = b + lane; t < e; t += 64) {
            const int j = ci[t];
            if (j == i) dii = va[t];
            if (j >= nf) first = min(first, t);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            dii += __shfl_xor(dii, d);  // one lane holds it
            first = min(first, __shfl_xor(first, d));
        }
        const double nd = -dii;
        double s = 1.0;
        if (isnsp == 1) {
            double acc = 0.0;
            if (lane == 0)
                for (int t = first; t < e; ++t) acc = acc + va[t] / nd;
            s = __shfl(acc, 0);
        }
        for (int t = first + lane; t < e; t += 64) {
            const double w = va[t] / nd;
            pci[pos0 + (t - first)] = ci[t] - nf;
            pva[pos0 + (t - first)] = isnsp == 1 ? w / s : w;
        }
        if (lane == 0) cmask[i] = 0;
    }
}

// General level (transfer.m:41-63).  One single-wave workgroup per row keeps two
// dense coarse rows in LDS: acc1 = W1(i,:) = Afc(i,:)/(-a_ii), acc2 = W2(i,:) =
// sum_k X(i,k) W1(k,:) with X = ((-Dff)\(Aff.*(I+As_FF))), k ascending; the row of
// W is W1 + 0.5*W2 (the always-true test at transfer.m:54).
__global__ __launch_bounds__(256) void k_build_W(int N, int Nc, const int* __restrict__ rp,
                                                const int* __restrict__ ci,
                                                const double* __restrict__ va,
                                                const double* __restrict__ diag,
                                                const uint8_t* __restrict__ strong,
                                                const uint8_t* __restrict__ isC,
                                                const uint8_t* __restrict__ isF,
                                                const int* __restrict__ cidx,
                                                double* __restrict__ dense,
                                                int* __restrict__ rowcnt) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* acc2 = reinterpret_cast<double*>(smem_raw);
    double* acc1 = acc2 + Nc;
    const int lane = threadIdx.x, T = blockDim.x;  // 64 or 256 threads per row
    __shared__ int wcnt[4];
    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        double* drow = dense + (size_t)i * Nc;
        if (isC[i]) {  // identity row of P = [W; I]
            const int me = cidx[i];
            for (int c = lane; c < Nc; c += T) drow[c] = (c == me) ? 1.0 : 0.0;
            if (lane == 0) rowcnt[i] = 1;
            continue;
        }
        for (int c = lane; c < Nc; c += T) {
            acc1[c] = 0.0;
            acc2[c] = 0.0;
        }
        __syncthreads();
        const double ndi = -diag[i];
        const int b = rp[i], e = rp[i + 1];
        for (int t = b + lane; t < e; t += T) {
            const int j = ci[t];
            if (isC[j]) acc1[cidx[j]] = va[t] / ndi;
        }
        for (int t = b; t < e; ++t) {
            const int k = ci[t];
            if (isF[k] && (k == i || strong[t])) {
                const double x = va[t] / ndi;
                const double ndk = -diag[k];
                for (int u = rp[k] + lane; u < rp[k + 1]; u += T) {
                    const int j = ci[u];
                    if (isC[j]) {
                        const double w1 = va[u] / ndk;
                        const double prod = x * w1;
                        const int c = cidx[j];
                        acc2[c] = acc2[c] + prod;
                    }
                }
                __syncthreads();
            }
        }
        __syncthreads();
        int nz = 0;
        for (int c = lane; c < Nc; c += T) {
            const double half = 0.5 * acc2[c];
            const double v = acc1[c] + half;
            drow[c] = v;
            nz += (v != 0.0);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) nz += __shfl_xor(nz, d);
        if ((lane & 63) == 0) wcnt[lane >> 6] = nz;
        __syncthreads();
        if (lane == 0) {
            int tot = 0;
            for (int w = 0; w < (T >> 6); ++w) tot += wcnt[w];
            rowcnt[i] = tot;   // (plain counts: the compaction or a scan launch turns them into row pointers)
        }
        __syncthreads();
    }
}

// The same rows with ONE WAVE per row, pipelined (the form of k_spgemm_rows_w).  k_build_W's loop over the
// strong F neighbours k is a chain of four dependent global round trips and a barrier per neighbour -- column,
// then diag / row range of k, then k's entries, then their C flags and indices: 0.5 us each, 44 us for the
// 90-entry rows of a 100-row level.  Here the lanes read the metadata of 64 entries of row i at once; the
// strong F neighbours are listed in LDS in ascending order, a row of k longer than 64 entries as up to four
// consecutive 64-entry pieces; and the pieces D ahead -- already filtered to C columns and divided by -a_kk --
// are in flight while the current D are applied.  Every acc2[c] still receives x(i,k) * w1(k,c) one term at a
// time in ascending k (the pieces of one k touch distinct columns), and a wave's LDS operations execute in
// program order: the bits equal k_build_W's.
constexpr int BW_PIECES = 4;   // 64-entry pieces of a neighbour's row that are prefetched (the rest: a plain loop)
template <int D>
__global__ __launch_bounds__(64) void k_build_W_w(int N, int Nc, const int* __restrict__ rp,
                                                  const int* __restrict__ ci,
                                                  const double* __restrict__ va,
                                                  const double* __restrict__ diag,
                                                  const uint8_t* __restrict__ strong,
                                                  const uint8_t* __restrict__ isC,
                                                  const uint8_t* __restrict__ isF,
                                                  const int* __restrict__ cidx,
                                                  double* __restrict__ dense,
                                                  int* __restrict__ rowcnt) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* acc2 = reinterpret_cast<double*>(smem_raw);
    double* acc1 = acc2 + Nc;
    __shared__ int s_yb[64 * BW_PIECES], s_yn[64 * BW_PIECES], s_te[64 * BW_PIECES];
    __shared__ double s_x[64 * BW_PIECES], s_nd[64 * BW_PIECES];
    const int lane = threadIdx.x;
    for (int i = blockIdx.x; i < N; i += gridDim.x) {
        double* drow = dense + (size_t)i * Nc;
        if (isC[i]) {  // identity row of P = [W; I]
            const int me = cidx[i];
            for (int c = lane; c < Nc; c += 64) drow[c] = (c == me) ? 1.0 : 0.0;
            if (lane == 0) rowcnt[i] = 1;
            continue;
        }
        for (int c = lane; c < Nc; c += 64) {
            acc1[c] = 0.0;
            acc2[c] = 0.0;
        }
        __syncthreads();
        const double ndi = -diag[i];
        const int b = rp[i], e = rp[i + 1];
        for (int e0 = b; e0 < e; e0 += 64) {
            const int t = e0 + lane;
            const bool mine = t < e;
            const int kk = mine ? ci[t] : 0;
            const double av = mine ? va[t] : 0.0;
            const bool kC = mine && isC[kk];
            const bool take = mine && isF[kk] && (kk == i || strong[t]);
            const double xq = av / ndi;                    // W1(i, .) entry or X(i, k)
            if (kC) acc1[cidx[kk]] = xq;
            // the strong F neighbours of this batch in ascending order, a row of more than 64 entries as pieces
            const int yb0 = take ? rp[kk] : 0;
            const int ylen = take ? rp[kk + 1] - yb0 : 0;
            const int npc = take ? min(BW_PIECES, (ylen + 63) >> 6) : 0;
            int r0 = npc;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(r0, d);
                if (lane >= d) r0 += y;
            }
            const int cnt = __shfl(r0, 63);
            r0 -= npc;
            if (take) {
                const double ndk = -diag[kk];
                for (int c = 0; c < npc; ++c) {
                    s_yb[r0 + c] = yb0 + 64 * c;
                    s_yn[r0 + c] = min(64, ylen - 64 * c);
                    s_te[r0 + c] = (c == npc - 1 && ylen > 64 * BW_PIECES) ? yb0 + ylen : 0;
                    s_x[r0 + c] = xq;
                    s_nd[r0 + c] = ndk;
                }
            }
            __syncthreads();
            int jA[D], jB[D], tA[D], tB[D];
            double vA[D], vB[D], xA[D], xB[D];
            // pieces u0 .. u0+D-1: C column index (or -1) and w1 = a_kj / -a_kk of the lane's entry; x(i,k) and the
            // long-row mark ride along, so that applying a piece is one LDS read-add-write and nothing else
            // (branch-free in two rounds -- all the pieces' entries, then all their C flags and indices -- so that the
            // D pieces' dependent loads overlap: under `if (lane < n) { j = ...; if (isC[j]) ... }` each piece
            // waited for its own two round trips in turn, 1.5 us per call)
            auto load = [&](int u0, int* jj, double* vv, double* xs, int* ts) __attribute__((always_inline)) {
                int jt[D], nn[D];
                double nd[D];
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int u = min(u0 + d, cnt - 1);   // uniform; cnt > 0 here
                    const int bb = s_yb[u];
                    nn[d] = u0 + d < cnt ? s_yn[u] : 0;
                    xs[d] = s_x[u];
                    ts[d] = u0 + d < cnt ? s_te[u] : 0;
                    nd[d] = s_nd[u];
                    const int idx = bb + min(lane, max(nn[d], 1) - 1);
                    jt[d] = ci[idx];
                    vv[d] = va[idx];
                }
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const bool c = isC[jt[d]] != 0;
                    const int cd = cidx[jt[d]];
                    jj[d] = (lane < nn[d] && c) ? cd : -1;
                    vv[d] = vv[d] / nd[d];
                }
            };
            auto apply = [&](int u0, const int* jj, const double* vv, const double* xs, const int* ts)
                             __attribute__((always_inline)) {
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const int u = u0 + d;   // uniform
                    if (u < cnt) {
                        const double x = xs[d];
                        if (jj[d] >= 0) {
                            const double prod = x * vv[d];
                            acc2[jj[d]] = acc2[jj[d]] + prod;
                        }
                        const int te = ts[d];
                        if (te) {   // the rest of a very long row (distinct columns: lane order is free)
                            const double ndk = s_nd[u];
                            for (int q = s_yb[u] + 64 + lane; q < te; q += 64) {
                                const int j = ci[q];
                                if (isC[j]) {
                                    const double w1 = va[q] / ndk;
                                    const double prod = x * w1;
                                    const int c = cidx[j];
                                    acc2[c] = acc2[c] + prod;
                                }
                            }
                        }
                    }
                }
            };
            if (cnt > 0) {
                load(0, jA, vA, xA, tA);
                for (int u0 = 0; u0 < cnt; u0 += 2 * D) {
                    load(u0 + D, jB, vB, xB, tB);
                    apply(u0, jA, vA, xA, tA);
                    load(u0 + 2 * D, jA, vA, xA, tA);
                    apply(u0 + D, jB, vB, xB, tB);
                }
            }
            __syncthreads();   // (the lists are rewritten by the next batch)
        }
        int nz = 0;
        for (int c = lane; c < Nc; c += 64) {
            const double half = 0.5 * acc2[c];
            const double v = acc1[c] + half;
            drow[c] = v;
            nz += (v != 0.0);
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) nz += __shfl_xor(nz, d);
        if (lane == 0) rowcnt[i] = nz;
        __syncthreads();
    }
}

// The same rows through the ordered product of ipd_sparse.hip, for levels whose rows are long
// (filled-in level 2 under dense masks): W1 and X are written as CSR matrices over all N rows
// (C rows empty), W2 = X*W1 is one csr_spgemm (which switches to register tiles when that is
// faster), and the rows of W are put together in a dense scratch.  Every W2(i,c) still receives
// x(i,k)*w1(k,c) one term at a time in ascending k, so the bits equal k_build_W's.
__global__ __launch_bounds__(256) void k_w_split_count(int N, const int* __restrict__ rp,
                                                      const int* __restrict__ ci,
                                                      const uint8_t* __restrict__ strong,
                                                      const uint8_t* __restrict__ isC,
                                                      const uint8_t* __restrict__ isF,
                                                      int* cnt1,
                                                      int* cntx, const ScanTail st) {
    WAVE_ROWS(i, N) {
        int n1 = 0, nx = 0;
        if (!isC[i])
            for (int t = rp[i] + lane; t < rp[i + 1]; t += 64) {
                const int j = ci[t];
                n1 += isC[j] != 0;
                nx += isF[j] && (j == i || strong[t]);
            }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            n1 += __shfl_xor(n1, d);
            nx += __shfl_xor(nx, d);
        }
        if (lane == 0) {
            if (st.out) {
                scan_put(cnt1, i, n1);
                scan_put(cntx, i, nx);
            } else {
                cnt1[i] = n1;
                cntx[i] = nx;
            }
        }
    }
    scan_tail(st);   // the row pointers of W1 and X, both totals in one mailbox message
}

__global__ __launch_bounds__(256) void k_w_split_fill(int N, const int* __restrict__ rp,
                                                     const int* __restrict__ ci,
                                                     const double* __restrict__ va,
                                                     const double* __restrict__ diag,
                                                     const uint8_t* __restrict__ strong,
                                                     const uint8_t* __restrict__ isC,
                                                     const uint8_t* __restrict__ isF,
                                                     const int* __restrict__ cidx,
                                                     const int* rp1,
                                                     int* __restrict__ ci1, double* __restrict__ va1,
                                                     const int* rpx,
                                                     int* __restrict__ cix, double* __restrict__ vax,
                                                     const int* __restrict__ head1,
                                                     const int* __restrict__ headx, int* rp1_out,
                                                     int* rpx_out) {
    // head1 != NULL: rp1 / rpx are still k_w_split_count's plain counts, scanned here (scan_head; N <= SCAN_HEAD_MAX)
    __shared__ ScanHeadLds L1, Lx;
    if (head1) {
        scan_head(head1, N, rp1_out, nullptr, L1);
        scan_head(headx, N, rpx_out, nullptr, Lx);
        rp1 = L1.rp;
        rpx = Lx.rp;
    }
    WAVE_ROWS(i, N) {
        if (isC[i]) continue;
        const double ndi = -diag[i];
        int b1 = rp1[i], bx = rpx[i];
        const int b = rp[i], e = rp[i + 1];
        for (int t0 = b; t0 < e; t0 += 64) {
            const int t = t0 + lane;
            const int j = t < e ? ci[t] : 0;
            const bool f1 = t < e && isC[j];
            const bool fx = t < e && isF[j] && (j == i || strong[t]);
            const double v = t < e ? va[t] / ndi : 0.0;
            const unsigned long long m1 = __ballot(f1), mx = __ballot(fx);
            const unsigned long long below = (1ull << lane) - 1ull;
            if (f1) {
                const int pos = b1 + __popcll(m1 & below);
                ci1[pos] = cidx[j];
                va1[pos] = v;
            }
            if (fx) {
                const int pos = bx + __popcll(mx & below);
                cix[pos] = j;
                vax[pos] = v;
            }
            b1 += __popcll(m1);
            bx += __popcll(mx);
        }
    }
}

// dense rows hold W1; add half of W2 on the F rows, write the identity entry on the C rows
__global__ __launch_bounds__(256) void k_w_combine(int N, int Nc, const uint8_t* __restrict__ isC,
                                                  const int* __restrict__ cidx,
                                                  const int* __restrict__ rp2,
                                                  const int* __restrict__ ci2,
                                                  const double* __restrict__ va2,
                                                  double* __restrict__ dense) {
    WAVE_ROWS(i, N) {
        double* drow = dense + (size_t)i * Nc;
        if (isC[i]) {
            if (lane == 0) drow[cidx[i]] = 1.0;
            continue;
        }
        for (int t = rp2[i] + lane; t < rp2[i + 1]; t += 64) {
            const int c = ci2[t];
            const double half = 0.5 * va2[t];
            drow[c] = drow[c] + half;
        }
    }
}

// dense rows -> CSR, one wave per row.  normF != NULL: D = diag(W*1); W = D\W on the F rows (transfer.m:60-62) --
// the row sum runs over the stored entries one at a time in ascending column order (the order MATLAB's sum over
// a sparse row takes), read out of the lanes that hold them.
__device__ __forceinline__ double su_readlane(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                            __builtin_amdgcn_readlane(__double2loint(v), l));
}
__global__ __launch_bounds__(256) void k_dense_compact2(int nr, int nc,
                                                        const double* __restrict__ dense,
                                                        const int* rp,
                                                        int* __restrict__ ci,
                                                        double* __restrict__ va,
                                                        const int* __restrict__ head_cnt, int* head_rp,
                                                        int* head_total,
                                                        const uint8_t* __restrict__ normF) {
    __shared__ ScanHeadLds L;   // head_cnt != NULL: plain counts, scanned here (scan_head; nr <= SCAN_HEAD_MAX)
    if (head_cnt) {
        scan_head(head_cnt, nr, head_rp, head_total, L);
        rp = L.rp;
    }
    WAVE_ROWS(i, nr) {
        int base = rp[i];
        const double* drow = dense + (size_t)i * nc;
        double s = 1.0;
        const bool norm = normF && normF[i];
        if (norm) {
            double acc = 0.0;
            for (int j0 = 0; j0 < nc; j0 += 64) {
                const int j = j0 + lane;
                const double v = j < nc ? drow[j] : 0.0;
                unsigned long long mask = __ballot(v != 0.0);
                while (mask) {
                    const int l = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    acc = acc + su_readlane(v, l);
                }
            }
            s = acc;
        }
        for (int j0 = 0; j0 < nc; j0 += 64) {
            const int j = j0 + lane;
            const double v = j < nc ? drow[j] : 0.0;
            const bool nzf = v != 0.0;
            const unsigned long long mask = __ballot(nzf);
            if (nzf) {
                const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
                ci[pos] = j;
                va[pos] = norm ? v / s : v;
            }
            base += __popcll(mask);
        }
    }
}

// ideal interpolation (transfer.m:57-58): Aff and Afc as dense row-major arrays, one wave per row
__global__ __launch_bounds__(256) void k_ideal_split(int N, int Nf, int Nc, const int* __restrict__ rp,
                                                     const int* __restrict__ ci,
                                                     const double* __restrict__ va,
                                                     const uint8_t* __restrict__ isF,
                                                     const int* __restrict__ fidx,
                                                     const int* __restrict__ cidx,
                                                     double* __restrict__ Aff, double* __restrict__ Afc) {
    WAVE_ROWS(i, N) {
        if (!isF[i]) continue;
        const size_t r = (size_t)fidx[i];
        for (int t = rp[i] + lane; t < rp[i + 1]; t += 64) {
            const int j = ci[t];
            if (isF[j])
                Aff[r * Nf + fidx[j]] = va[t];
            else
                Afc[r * Nc + cidx[j]] = va[t];
        }
    }
}
// rows of Pro in the original ordering: F rows = -(Aff \ Afc), C rows = identity (Pro(p,:) = P, :63)
__global__ void k_ideal_rows(int N, int Nc, const uint8_t* __restrict__ isF, const int* __restrict__ fidx,
                             const int* __restrict__ cidx, const double* __restrict__ X,
                             double* __restrict__ dense) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < (size_t)N * Nc;
         e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e / Nc), c = (int)(e % Nc);
        dense[e] = isF[i] ? -X[(size_t)fidx[i] * Nc + c] : (c == cidx[i] ? 1.0 : 0.0);
    }
}

// ---------------------------------------------------------------------------
// P of a level, from its plan
// ---------------------------------------------------------------------------
void amg_prolong_bigraph(ipd_ctx* ctx, Arena& dst, const Csr& A, const AmgOpts& o, const TransferPlan& plan,
                         int* counts, uint8_t* cmask, Csr* Pout) {                // transfer.m:19-25
    const int N = A.nr, nf = (int)o.fnode;
    Csr P;
    P.nr = N;
    P.nc = N - nf;
    P.rp = dst.alloc<int>((size_t)N + 1);
    // lazy: the fill scans the plain row lengths itself, P's arrays are sized by A's entry count, and count and
    // "Aff is not diagonal" flag are fetched with the products' counts.  Otherwise entry count and flag come with
    // the count launch's tail: one launch, ONE round trip.
    RowCounts rc(ctx, plan.p_rows, N, P.rp, counts);
    hipLaunchKernelGGL(k_bigph_count, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, nf, A.rp, A.ci, rc.cnt,
                       rc.tail, plan.lazy ? counts + 3 : (int*)nullptr);
    IPD_KERNEL_CHECK();
    int notdiag = 0;
    P.nnz = rc.finish(plan.p_bound, &notdiag);
    IPD_REQUIRE(notdiag == 0, IPD_E_UNSUPPORTED,
                "transfer: bigph level 1 needs a diagonal Aff block (transfer.m:20-21)");
    const int* head = rc.head();
    P.ci = dst.alloc<int>((size_t)P.nnz);
    P.va = dst.alloc<double>((size_t)P.nnz);
    hipLaunchKernelGGL(k_bigph_fill, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, nf,
                       o.isnsp, A.rp, A.ci, A.va, (const int*)P.rp, P.ci, P.va, cmask, head, P.rp,
                       head ? counts : (int*)nullptr);
    IPD_KERNEL_CHECK();
    *Pout = P;
}

// W = -Aff \ Afc as dense rows (transfer.m:57-58).  MATLAB solves with the sparse Aff (CHOLMOD); here a dense
// Cholesky of the F-F block (a principal block of the SPD level matrix) with the Nc columns of Afc as right-hand
// sides (csrc/ipd_dense.hip).  Cold path.
static void ideal_rows(ipd_ctx* ctx, const Csr& A, const LevelSplit& s, double* dense) {
    Arena& tmp = *ctx->scratch;
    const int N = A.nr, Nc = s.Nc, Nf = N - Nc;
    IPD_REQUIRE((size_t)Nf * Nf * 8 <= DENSE_SCRATCH_BYTES_MAX, IPD_E_LIMIT,
                "transfer: dense Aff of the ideal interpolation above 2 GiB");
    int* fflag = tmp.alloc<int>((size_t)N + 1);
    int* fidx = tmp.alloc<int>((size_t)N + 1);
    amg_mask_index(ctx, s.isF, fflag, fidx, N);
    double* Aff = tmp.alloc<double>((size_t)std::max(Nf, 1) * std::max(Nf, 1));
    double* Afc = tmp.alloc<double>((size_t)std::max(Nf, 1) * Nc);
    IPD_HIP(hipMemsetAsync(Aff, 0, sizeof(double) * (size_t)Nf * Nf, ctx->stream));
    IPD_HIP(hipMemsetAsync(Afc, 0, sizeof(double) * (size_t)Nf * Nc, ctx->stream));
    if (Nf > 0) {
        hipLaunchKernelGGL(k_ideal_split, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, Nf, Nc,
                           A.rp, A.ci, A.va, s.isF, fidx, s.cidx, Aff, Afc);
        IPD_KERNEL_CHECK();
        dense_chol_factor(ctx, Aff, Nf, Nf);
        dense_chol_solve(ctx, Aff, Nf, Nf, Afc, Nc, Nc);
    }
    const size_t dense_elems = (size_t)N * (size_t)Nc;
    hipLaunchKernelGGL(k_ideal_rows, dim3((int)std::min<size_t>((dense_elems + 255) / 256, 8192)),
                       dim3(256), 0, ctx->stream, N, Nc, s.isF, fidx, s.cidx, (const double*)Afc, dense);
    IPD_KERNEL_CHECK();
}

// The classical rows through the ordered product (see k_w_split_count); dense starts out as zeros.  `head`: P's
// count is lazy and the level small enough for head scans.
static void split_rows(ipd_ctx* ctx, const Csr& A, const LevelSplit& s, bool head, double* dense) {
    Arena& tmp = *ctx->scratch;
    const int N = A.nr, Nc = s.Nc;
    Csr W1, X, W2;
    W1.nr = N;
    W1.nc = Nc;
    X.nr = X.nc = N;
    W1.rp = tmp.alloc<int>((size_t)N + 1);
    X.rp = tmp.alloc<int>((size_t)N + 1);
    // head: no round trip -- W1 and X are sub-patterns of A (arrays sized by A's entry count, the fill scans the
    // plain counts itself) and the product's count stays on the device.  Otherwise counts, both scans and both
    // totals are one launch and one round trip (a ScanTail over two arrays: not RowCounts' case).
    int* cnt1 = head ? tmp.alloc<int>((size_t)N + 1) : zeroed<int>(ctx, (size_t)N + 1);
    int* cntx = head ? tmp.alloc<int>((size_t)N + 1) : zeroed<int>(ctx, (size_t)N + 1);
    std::unique_ptr<TailTotal> wt;
    if (!head) {
        wt.reset(new TailTotal(ctx, cnt1, W1.rp, N));
        wt->t.in2 = cntx;
        wt->t.out2 = X.rp;
    }
    hipLaunchKernelGGL(k_w_split_count, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, A.rp, A.ci, s.strong,
                       s.isC, s.isF, cnt1, cntx, head ? ScanTail() : wt->t);
    IPD_KERNEL_CHECK();
    int t[2] = {std::max(A.nnz, 1), std::max(A.nnz, 1)};   // (allocation bound)
    if (!head) wt->wait(t);
    W1.nnz = t[0];
    X.nnz = t[1];
    W1.ci = tmp.alloc<int>((size_t)std::max(W1.nnz, 1));
    W1.va = tmp.alloc<double>((size_t)std::max(W1.nnz, 1));
    X.ci = tmp.alloc<int>((size_t)std::max(X.nnz, 1));
    X.va = tmp.alloc<double>((size_t)std::max(X.nnz, 1));
    hipLaunchKernelGGL(k_w_split_fill, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, A.rp, A.ci, A.va, s.diag,
                       s.strong, s.isC, s.isF, s.cidx, (const int*)W1.rp, W1.ci, W1.va, (const int*)X.rp, X.ci, X.va,
                       head ? (const int*)cnt1 : nullptr, head ? (const int*)cntx : nullptr, head ? W1.rp : nullptr,
                       head ? X.rp : nullptr);
    IPD_KERNEL_CHECK();
    if (head) {
        W1.nnz = X.nnz = std::max(A.nnz / 2, 1);   // (estimates for the product's kernel choice)
        csr_spgemm(ctx, tmp, X, W1, &W2, tmp.alloc<int>(1));
    } else
        csr_spgemm(ctx, tmp, X, W1, &W2);
    csr_expand_dense(ctx, W1, dense, Nc);
    hipLaunchKernelGGL(k_w_combine, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, Nc, s.isC,
                       s.cidx, W2.rp, W2.ci, W2.va, dense);
    IPD_KERNEL_CHECK();
}

void amg_prolong_classical(ipd_ctx* ctx, Arena& dst, const Csr& A, const AmgOpts& o, const TransferPlan& plan,
                           const LevelSplit& s, int* counts, Csr* Pout) {          // transfer.m:41-63
    Arena& tmp = *ctx->scratch;
    const int N = A.nr, Nc = s.Nc;
    Csr P;
    P.nr = N;
    P.nc = Nc;
    const size_t dense_elems = (size_t)N * (size_t)Nc;
    IPD_REQUIRE(dense_elems * 8 <= DENSE_SCRATCH_BYTES_MAX, IPD_E_LIMIT,
                "transfer: dense interpolation scratch above 2 GiB");
    // (the product form adds into rows that start out as zeros)
    double* dense = plan.form == FORM_SPLIT ? zeroed<double>(ctx, dense_elems) : tmp.alloc<double>(dense_elems);
    // P's row pointers: the ideal and the product form count the dense rows in a 256-thread launch that can
    // carry a tail; k_build_W(_w) leave plain counts
    P.rp = dst.alloc<int>((size_t)N + 1);
    RowCounts rc(ctx, plan.p_rows, N, P.rp, counts);
    switch (plan.form) {
        case FORM_IDEAL:
            ideal_rows(ctx, A, s, dense);
            dense_rowcount(ctx, N, Nc, Nc, dense, rc.cnt, rc.tail);
            break;
        case FORM_SPLIT:
            split_rows(ctx, A, s, plan.p_rows == RC_HEAD, dense);
            dense_rowcount(ctx, N, Nc, Nc, dense, rc.cnt, rc.tail);
            break;
        case FORM_BLOCK:
            IPD_OPTIN_LDS(ctx, k_build_W, 128 * 1024);
            hipLaunchKernelGGL(k_build_W, dim3(std::min(N, 16384)), dim3(plan.block_threads), (size_t)Nc * 16,
                               ctx->stream, N, Nc, A.rp, A.ci, A.va, s.diag, s.strong, s.isC, s.isF, s.cidx, dense,
                               rc.cnt);
            IPD_KERNEL_CHECK();
            break;
        default:
            IPD_OPTIN_LDS(ctx, k_build_W_w<8>, 128 * 1024);
            hipLaunchKernelGGL(k_build_W_w<8>, dim3(std::min(N, 16384)), dim3(64), (size_t)Nc * 16, ctx->stream,
                               N, Nc, A.rp, A.ci, A.va, s.diag, s.strong, s.isC, s.isF, s.cidx, dense, rc.cnt);
            IPD_KERNEL_CHECK();
    }
    P.nnz = rc.finish(plan.p_bound);
    const int* head = rc.head();   // plain counts the compaction scans itself
    P.ci = dst.alloc<int>((size_t)std::max(P.nnz, 1));
    P.va = dst.alloc<double>((size_t)std::max(P.nnz, 1));
    // compaction, and D = diag(W*1); W = D\W on the F rows (transfer.m:60-62) in the same launch
    hipLaunchKernelGGL(k_dense_compact2, dim3(rows_grid(N)), dim3(256), 0, ctx->stream, N, Nc,
                       dense, (const int*)P.rp, P.ci, P.va, head, P.rp, head ? counts : (int*)nullptr,
                       o.isnsp == 1 ? (const uint8_t*)s.isF : (const uint8_t*)nullptr);
    IPD_KERNEL_CHECK();
    *Pout = P;
}
