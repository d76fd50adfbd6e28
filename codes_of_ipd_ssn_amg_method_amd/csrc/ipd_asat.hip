// The active-set KKT assembly ASAt.m:14-19 (the matrix-free operators beside it: ipd_kkt.hip).
//
// Layout: s is m*n column-major (Y(i,j) = s[i + j*m]); the KKT unknowns
// are ordered [0,n) = column constraints, [n,n+m) = row constraints
// (Class1/APD_SsN_Class1.m:33).
//
// Roofline: a single streaming pass -> HBM bound.
//   ASAt : m*n (mask) + 8*(m+n) + 16*(2E+M) bytes
// This TU is compiled with -ffp-contract=off so that the ASAt values
// are bit-identical to the oracle (two multiplies and one add per entry).
// The route between the two assemblies, the capacity guess, the grids and the scratch sizes: ipd_kkt_plan.h.
#pragma clang fp contract(off)

#include "ipd_kkt.h"

// ---------------------------------------------------------------------------
// ASAt:  H = A*diag(s)*A'  as CSR (== MATLAB's CSC, H is symmetric)
// ---------------------------------------------------------------------------
// Row j < n      : [ (j,j) , (j, n+i) for every i with Y(i,j)=1, ascending i ]
// Row n+i        : [ (n+i, j) for every j with Y(i,j)=1, ascending j , (n+i,n+i) ]
// A diagonal entry exists iff its row has any off-diagonal (MATLAB stores no
// explicit zeros; a p or q whose square underflows to 0 is handled by a
// zero-dropping pass).
//
// The byte mask is read once, as 64x64 tiles, one tile per wave: a wave ballot
// turns the 64 bytes of a column into a 64-bit row mask; 64 more ballots
// transpose the tile into per-row column masks.  Both bit-packed copies
// (2*m*n/8 bytes) are kept so the fill pass never touches the bytes again.
struct AsatPlan {
    int m, n, nib, njb;
    unsigned long long* colmask;  // [nib][n]  bits = rows of the tile
    unsigned long long* rowmask;  // [njb][m]  bits = columns of the tile
    int* coloff;                  // [nib][n]  entries of column j in tiles above
    int* rowoff;                  // [njb][m]
    int* cntc;                    // [n]
    int* cntr;                    // [m]
    int* rowlen;                  // [n+m]
};

// WIDE: m % 8 == 0 and s 8-byte aligned -- lane l reads the 64 bytes of column j0+l as eight
// 8-byte words and packs each to 8 bits (nonzero byte -> bit), so the lane's column mask needs
// no ballot; otherwise byte loads + one ballot per column.
__device__ __forceinline__ unsigned bytes_to_bits(unsigned long long x) {
    x |= x >> 4;
    x |= x >> 2;
    x |= x >> 1;
    x &= 0x0101010101010101ull;
    return (unsigned)((x * 0x0102040810204080ull) >> 56);
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_asat_masks(const uint8_t* __restrict__ s, AsatPlan pl) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= pl.nib * pl.njb) return;
    const int ib = tile % pl.nib, jb = tile / pl.nib;
    const int i0 = ib * 64, j0 = jb * 64;
    const int i = i0 + lane;
    unsigned long long colm = 0ull;
    if (WIDE && i0 + 64 <= pl.m) {
        const int j = j0 + lane;
        const unsigned long long* src =
            reinterpret_cast<const unsigned long long*>(s + (size_t)(j < pl.n ? j : 0) * pl.m + i0);
        unsigned long long wd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) wd[k] = src[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) colm |= (unsigned long long)bytes_to_bits(wd[k]) << (8 * k);
        if (j >= pl.n) colm = 0ull;
    } else {
#pragma unroll 8
        for (int jj = 0; jj < 64; ++jj) {
            const int j = j0 + jj;
            uint8_t b = 0;
            if (i < pl.m && j < pl.n) b = s[(size_t)j * pl.m + i];
            const unsigned long long mk = __ballot(b != 0);
            if (lane == jj) colm = mk;
        }
    }
    unsigned long long rowm = 0ull;
#pragma unroll 8
    for (int b = 0; b < 64; ++b) {
        const unsigned long long mk = __ballot((colm >> b) & 1ull);
        if (lane == b) rowm = mk;
    }
    if (j0 + lane < pl.n) pl.colmask[(size_t)ib * pl.n + j0 + lane] = colm;
    if (i < pl.m) pl.rowmask[(size_t)jb * pl.m + i] = rowm;
}

// per column / per row: running offsets over the tiles, counts, H row lengths,
// and the "some p_i^2 or q_j^2 is exactly zero" flag (meta[1]).
__global__ __launch_bounds__(256) void k_asat_offsets(AsatPlan pl, const double* __restrict__ p,
                                                      const double* __restrict__ q,
                                                      int* __restrict__ meta_flag) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < pl.n) {
        int run = 0;
        for (int ib = 0; ib < pl.nib; ++ib) {
            pl.coloff[(size_t)ib * pl.n + t] = run;
            run += __popcll(pl.colmask[(size_t)ib * pl.n + t]);
        }
        pl.cntc[t] = run;
        pl.rowlen[t] = run + (run > 0 ? 1 : 0);
        const double qq = q[t] * q[t];
        if (qq == 0.0) *meta_flag = 1;
    } else if (t < pl.n + pl.m) {
        const int i = t - pl.n;
        int run = 0;
        for (int jb = 0; jb < pl.njb; ++jb) {
            pl.rowoff[(size_t)jb * pl.m + i] = run;
            run += __popcll(pl.rowmask[(size_t)jb * pl.m + i]);
        }
        pl.cntr[i] = run;
        pl.rowlen[t] = run + (run > 0 ? 1 : 0);
        const double pp = p[i] * p[i];
        if (pp == 0.0) *meta_flag = 1;
    }
}

// Off-diagonal entries.  One wave per 64x64 tile; for every column (then every row) of the tile
// that has entries, lane b owns bit b of its mask word and writes its entry at the word's base
// position + the number of set bits below b: the 64 stores of a step are consecutive entries
// (one lane walking its own row wrote with a stride of a whole row: 50 us at rho = 1, m=n=1024,
// for 25 MB; this takes 9).
__device__ __forceinline__ unsigned long long wave_bcast64(unsigned long long v, int srclane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, srclane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), srclane);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ double wave_bcast_f64(double v, int srclane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), srclane),
                            __builtin_amdgcn_readlane(__double2loint(v), srclane));
}

__global__ __launch_bounds__(256) void k_asat_fill(AsatPlan pl, const double* __restrict__ p,
                                                   const double* __restrict__ q,
                                                   const int* __restrict__ rp,
                                                   int* __restrict__ ci, double* __restrict__ va,
                                                   int cap /* entries allocated */) {
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= pl.nib * pl.njb) return;
    const int ib = tile % pl.nib, jb = tile / pl.nib;
    const int i0 = ib * 64, j0 = jb * 64;
    const int il = i0 + lane, jl = j0 + lane;
    const bool iok = il < pl.m, jok = jl < pl.n;
    const unsigned long long colm = jok ? pl.colmask[(size_t)ib * pl.n + jl] : 0ull;
    const unsigned long long rowm = iok ? pl.rowmask[(size_t)jb * pl.m + il] : 0ull;
    const int cpos = jok ? rp[jl] + 1 + pl.coloff[(size_t)ib * pl.n + jl] : 0;
    const int rpos = iok ? rp[pl.n + il] + pl.rowoff[(size_t)jb * pl.m + il] : 0;
    const double pv = iok ? p[il] : 0.0, qv = jok ? q[jl] : 0.0;
    const unsigned long long below = (1ull << lane) - 1ull;
    // rows [0,n): column j of Y -> entries (j, n+i), ascending i
    for (unsigned long long nz = __ballot(colm != 0ull); nz; nz &= nz - 1ull) {
        const int jj = __ffsll((long long)nz) - 1;
        const unsigned long long cm = wave_bcast64(colm, jj);
        const int pos0 = __builtin_amdgcn_readlane(cpos, jj);
        const double qj = wave_bcast_f64(qv, jj);
        if ((cm >> lane) & 1ull) {
            const int pos = pos0 + __popcll(cm & below);
            if (pos < cap) {
                ci[pos] = pl.n + il;
                va[pos] = qj * pv;   // q_j * (p_i * Y_ij)
            }
        }
    }
    // rows [n,n+m): row i of Y -> entries (n+i, j), ascending j
    for (unsigned long long nz = __ballot(rowm != 0ull); nz; nz &= nz - 1ull) {
        const int ii = __ffsll((long long)nz) - 1;
        const unsigned long long rm = wave_bcast64(rowm, ii);
        const int pos0 = __builtin_amdgcn_readlane(rpos, ii);
        const double pi = wave_bcast_f64(pv, ii);
        if ((rm >> lane) & 1ull) {
            const int pos = pos0 + __popcll(rm & below);
            if (pos < cap) {
                ci[pos] = jl;
                va[pos] = pi * qv;   // p_i * (Y_ij * q_j)
            }
        }
    }
}

// Diagonal values, accumulated sequentially in ascending index order exactly as the sparse
// products U'*p and Q*q of ASAt.m:19 do.  The order of the ADDS is what the bits fix, not the
// order of the loads.  A lane owns one H row and walks the row's words of the bit mask (coalesced
// across the 64 rows of the wave; not the column indices the fill pass wrote, so no dependent
// gather); per tile, lane l squares entry l of p (or q) -- the next tile's already in flight --
// and the wave loops, with a scalar bit scan, over the bit positions ANY of its rows has: the
// square comes out of lane b's register (v_readlane), a row without the bit adds +0.0, which
// leaves its sum as it is.  Nothing but the mask words and the vector is read.
// (One lane per row walking ci[e] -> p[ci[e]] in memory took 439 us at rho = 1, m=n=1024.)
// Blocks [0, nbc) are the rows [0,n) (column sums, vector p), the others the rows [n,n+m).
__device__ __forceinline__ unsigned wave_or_u32(unsigned v) {
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true);
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true);
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__global__ __launch_bounds__(64) void k_asat_diag(AsatPlan pl, const double* __restrict__ p,
                                                  const double* __restrict__ q, int nbc,
                                                  const int* __restrict__ rp, int* __restrict__ ci,
                                                  double* __restrict__ va, int cap) {
    const int lane = threadIdx.x;
    const int side = blockIdx.x >= nbc ? 1 : 0;                 // uniform
    const int nrow = side ? pl.m : pl.n, len = side ? pl.n : pl.m;
    const int nt = side ? pl.njb : pl.nib;
    const double* __restrict__ vec = side ? q : p;
    const unsigned long long* __restrict__ masks = side ? pl.rowmask : pl.colmask;
    const int idx = (blockIdx.x - (side ? nbc : 0)) * 64 + lane;
    const bool live = idx < nrow;
    const int ic = live ? idx : 0;
    const int cnt = live ? (side ? pl.cntr[ic] : pl.cntc[ic]) : 0;
    double sum = 0.0;
    constexpr int CH = 8;    // tiles whose mask words and vector entries are requested together
    for (int t0 = 0; t0 < nt; t0 += CH) {
        unsigned long long wb[CH];
        double vb[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k;
            const bool tok = t < nt;
            const unsigned long long wv = masks[(size_t)(tok ? t : 0) * nrow + ic];
            const int e = t * 64 + lane;
            const double vv = vec[(tok && e < len) ? e : 0];
            wb[k] = (tok && live) ? wv : 0ull;
            vb[k] = vv;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const unsigned long long w = wb[k];
            const double sq = vb[k] * vb[k];          // (p_i*Y_ij) * p_i, (Y_ij*q_j) * q_j
            const int slo = __double2loint(sq), shi = __double2hiint(sq);
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const unsigned wh = half ? (unsigned)(w >> 32) : (unsigned)w;
                unsigned u = wave_or_u32(wh);         // scalar: positions any row of the wave has
                if (u == 0u) continue;
                if (u == 0xFFFFFFFFu) {
                    // every position present somewhere (dense masks): fixed lanes and bit numbers,
                    // no scalar bit scan; a row without the bit adds +0.0 (mask 0 / ~0 from the bit)
#pragma unroll
                    for (int bpos = 0; bpos < 32; ++bpos) {
                        const int m = __builtin_amdgcn_sbfe(wh, bpos, 1);
                        const int xl = __builtin_amdgcn_readlane(slo, half * 32 + bpos) & m;
                        const int xh = __builtin_amdgcn_readlane(shi, half * 32 + bpos) & m;
                        sum = sum + __hiloint2double(xh, xl);
                    }
                    continue;
                }
                if (__popc(u) <= 6) {
                    // few positions (the realistic, tree-like masks): every lane takes its own bits,
                    // the squares come from the owning lanes' registers (ds_bpermute, no memory)
                    unsigned mine = wh;
                    while (__any(mine != 0u)) {
                        const bool has = mine != 0u;
                        const int bpos = has ? __builtin_ctz(mine) : 0;
                        mine &= mine - 1u;            // 0 stays 0
                        const double y = __shfl(sq, half * 32 + bpos);
                        sum = sum + (has ? y : 0.0);
                    }
                    continue;
                }
                while (u) {
                    const int bpos = __builtin_ctz(u);
                    u &= u - 1u;
                    const int m = __builtin_amdgcn_sbfe(wh, bpos, 1);
                    const int xl = __builtin_amdgcn_readlane(slo, half * 32 + bpos) & m;
                    const int xh = __builtin_amdgcn_readlane(shi, half * 32 + bpos) & m;
                    sum = sum + __hiloint2double(xh, xl);
                }
            }
        }
    }
    if (cnt > 0) {
        const int row = side ? pl.n + idx : idx;
        const int pos = rp[row] + (side ? cnt : 0);
        if (pos < cap) {
            ci[pos] = row;
            va[pos] = sum;
        }
    }
}


// Everything after the masks in ONE launch, for small active sets (the drivers' Newton systems:
// E ~ m + n, tree-like): a thread owns a row of H, counts its mask bits, the row pointers come from
// a scan inside the workgroup, and the thread then writes its row -- diagonal, off-diagonal entries
// in ascending column order, the diagonal value summed in ascending index order as ASAt.m:19's
// products do -- and the entry count goes to the host mailbox with the kernel's last store.  The
// general path above is six dependent launches and a read-back, 56-79 us whatever E is (launch-
// bound); this one is k_asat_masks + this kernel.  Same values, same order, same bits.
struct AsatSmallArgs {
    AsatPlan pl;
    const double* p;
    const double* q;
    int* rp;          // M + 2: rp[M] = nnz, rp[M+1] = zero-square flag
    int* ci;
    double* va;
    int cap;
    unsigned long long* agg;   // per workgroup: ticket << 32 | entries of its rows
    volatile unsigned* box;
    unsigned ticket;
};
// G = ceil(M / 256) workgroups of 256 rows; the row pointers come from a chained scan with look-back:
// a workgroup publishes the entry count of its rows, tagged with the call's ticket (so the words
// need no clearing between calls), as soon as it has it, reads the tagged counts of ALL its
// predecessors in one sweep (lane = predecessor, at most ASAT_SMALL_WGS of them) and repeats the sweep until every
// tag is there.  All workgroups are on the chip together (G <= 8 of 256 CUs: ipd_kkt_plan.h); the spin is bounded
// anyway, and a give-up is reported as an impossible count, which sends the host to the general path.
__global__ __launch_bounds__(256) void k_asat_small(const AsatSmallArgs a) {
    extern __shared__ __attribute__((aligned(16))) double asat_pq[];   // p (m), then q (n)
    __shared__ int wsum[4];
    __shared__ int s_flag, s_prefix, s_zpred;
    const AsatPlan& pl = a.pl;
    const int n = pl.n, m = pl.m, M = n + m, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = blockIdx.x, G = gridDim.x;
    const int t = g * 256 + tid;
    const bool frow = t < n, live = t < M;
    const int r = frow ? t : t - n;                               // column j of Y, or row i
    const int nw = frow ? pl.nib : pl.njb, stride = frow ? n : m;
    const unsigned long long* __restrict__ mk = frow ? pl.colmask : pl.rowmask;
    // one burst: the row's mask words, then p and q into LDS (the gathers of the fill)
    unsigned long long w[ASAT_SMALL_WORDS];   // asat_small_route: nib, njb <= ASAT_SMALL_WORDS
#pragma unroll
    for (int k = 0; k < ASAT_SMALL_WORDS; ++k) w[k] = (live && k < nw) ? mk[(size_t)k * stride + r] : 0ull;
    double* sp = asat_pq;
    double* sq = asat_pq + m;
    for (int i = tid; i < m; i += 256) sp[i] = a.p[i];
    for (int j = tid; j < n; j += 256) sq[j] = a.q[j];
    if (tid == 0) s_zpred = 0;
    int run = 0;
#pragma unroll
    for (int k = 0; k < ASAT_SMALL_WORDS; ++k) run += __popcll(w[k]);
    const int len = run + (run > 0 ? 1 : 0);
    int x = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wv] = x;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sgm = wsum[k];
        if (k < wv) woff += sgm;
        tot += sgm;
    }
    // publish this workgroup's count (bit 31: one of its rows has a zero square), then sum the predecessors'
    unsigned long long* agg = a.agg;
    {
        const double own0 = live ? (frow ? a.q[r] : a.p[r]) : 1.0;
        const int zs = __syncthreads_or(own0 * own0 == 0.0 ? 1 : 0);
        if (tid == 0) {
            s_flag = zs;
            __hip_atomic_store(&agg[g], ((unsigned long long)a.ticket << 32) | (unsigned)tot | (zs ? 0x80000000u : 0u),
                               __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (wv == 0) {
        static_assert(ASAT_SMALL_WGS == 64, "the sweep reads one predecessor per lane of one wave");
        int before = 0;
        bool ok = false;
        for (int spin = 0; spin < (1 << 20) && !ok; ++spin) {
            const unsigned long long v = lane < g ? __hip_atomic_load(&agg[lane], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
                                                  : ((unsigned long long)a.ticket << 32);
            const bool mine = (unsigned)(v >> 32) == a.ticket;
            ok = __all(mine);
            if (ok) {
                int c = lane < g ? (int)((unsigned)v & 0x7fffffffu) : 0;
                const int zb = __any(lane < g && ((unsigned)v >> 31)) ? 1 : 0;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
                before = c;
                if (lane == 0) s_zpred = zb;
            } else {
                __builtin_amdgcn_s_sleep(2);
            }
        }
        if (lane == 0) s_prefix = ok ? before : -1;
    }
    __syncthreads();
    const int carry = s_prefix;
    const bool gaveup = carry < 0;
    const int beg = (gaveup ? 0 : carry) + woff + x - len;
    if (live && !gaveup) a.rp[t] = beg;
    if (live && len > 0 && !gaveup) {
        // rows [0,n): diagonal first, then (j, n+i) ascending i;  rows [n,n+m): (n+i, j) ascending j,
        // diagonal last.  The diagonal value is summed in ascending index order (ASAt.m:19).
        const double own = frow ? sq[r] : sp[r];
        const double* other = frow ? sp : sq;
        int pos = frow ? beg + 1 : beg;
        double sum = 0.0;
#pragma unroll
        for (int k = 0; k < ASAT_SMALL_WORDS; ++k) {
            unsigned long long ww = w[k];
            while (ww) {
                const int o = k * ASAT_TILE + __builtin_ctzll(ww);
                ww &= ww - 1ull;
                const double ov = other[o];
                sum = sum + ov * ov;                               // (p_i*Y_ij)*p_i  /  (Y_ij*q_j)*q_j
                if (pos < a.cap) {
                    a.ci[pos] = frow ? n + o : o;
                    a.va[pos] = own * ov;                          // q_j*(p_i*Y_ij)  /  p_i*(Y_ij*q_j)
                }
                ++pos;
            }
        }
        const int dpos = frow ? beg : pos;
        if (dpos < a.cap) {
            a.ci[dpos] = t;
            a.va[dpos] = sum;
        }
    }
    if (g == G - 1) {   // the last workgroup knows the total and every workgroup's zero-square bit
        __syncthreads();
        if (tid == 0) {
            const int total = gaveup ? ASAT_GAVE_UP : carry + tot;
            const int zs = (s_flag || s_zpred) ? 1 : 0;
            a.rp[M] = total;
            a.rp[M + 1] = zs;
            a.box[16] = (unsigned)total;
            a.box[17] = (unsigned)zs;
            __threadfence_system();
            a.box[0] = a.ticket;
        }
    }
}

// ---------------------------------------------------------------------------
// the assembly: check, plan, masks, the one-launch route or the general one, finish
// ---------------------------------------------------------------------------
// what both routes work on
struct AsatJob {
    ipd_ctx* ctx;
    Arena& dst;      // H's arrays
    AsatGeo g;
    AsatPlan pl;
    const double *p, *q;
    int* rp;         // g.rp_len() entries: rp[M] = nnz, rp[M+1] = zero-square flag
    void clear_zflag() const { IPD_HIP(hipMemsetAsync(rp + g.M + 1, 0, sizeof(int), ctx->stream)); }
};

// the device plan over scratch; the braces fix the order of the allocations
static AsatPlan asat_scratch(Arena& tmp, const AsatGeo& g) {
    return AsatPlan{g.m, g.n, g.nib, g.njb,
                    tmp.alloc<unsigned long long>(g.col_words()), tmp.alloc<unsigned long long>(g.row_words()),
                    tmp.alloc<int>(g.col_words()), tmp.alloc<int>(g.row_words()),
                    tmp.alloc<int>((size_t)g.n), tmp.alloc<int>((size_t)g.m), tmp.alloc<int>((size_t)g.M)};
}

// Small active sets (the previous call's count says so): masks + ONE more launch, the count by mailbox.
// false: the active set grew beyond the guess (or a spin gave up) -- the arrays sized by the guess stay behind in
// dst and the general route redoes the assembly.
static bool asat_small(const AsatJob& j, unsigned ticket, Csr* h, bool* zero_squares) {
    ipd_ctx* ctx = j.ctx;
    const long long cap = asat_cap(ctx->asat_nnz_hint, j.g.m, j.g.n);
    h->ci = j.dst.alloc<int>((size_t)cap);
    h->va = j.dst.alloc<double>((size_t)cap);
    if (!ctx->asat_agg) {   // the tagged words, kept for the context's lifetime
        IPD_HIP(hipMalloc(&ctx->asat_agg, ASAT_SMALL_WGS * sizeof(unsigned long long)));
        IPD_HIP(hipMemsetAsync(ctx->asat_agg, 0, ASAT_SMALL_WGS * sizeof(unsigned long long), ctx->stream));
    }
    const AsatSmallArgs sa{j.pl, j.p, j.q, j.rp, h->ci, h->va, (int)cap,
                           static_cast<unsigned long long*>(ctx->asat_agg), ctx->mailbox, ticket};
    hipLaunchKernelGGL(k_asat_small, dim3(j.g.rows_grid()), dim3(256), j.g.small_lds(), ctx->stream, sa);
    IPD_KERNEL_CHECK();
    unsigned w2[2] = {0, 0};
    ctx->mailbox_wait(ticket, w2, sizeof(w2));
    h->nnz = (int)w2[0];
    *zero_squares = w2[1] != 0;
    ctx->asat_nnz_hint = asat_hint_after_small(ctx->asat_nnz_hint, h->nnz);
    if (asat_accepts(h->nnz, cap)) return true;
    j.clear_zflag();
    return false;
}

// The general route: offsets, scan, fill + diag.  The entry count sizes ci/va, and reading it back is a host round
// trip in the middle of the assembly.  Consecutive Newton steps have similar active sets, so the arrays are sized
// from the previous call's count (asat_cap) and the fill runs at once; the count is read afterwards, and only when
// it exceeds the guess (the kernels never write past `cap`) the fill is redone.
static void asat_general(const AsatJob& j, Csr* h, bool* zero_squares) {
    ipd_ctx* ctx = j.ctx;
    const AsatGeo& g = j.g;
    hipLaunchKernelGGL(k_asat_offsets, dim3(g.rows_grid()), dim3(256), 0, ctx->stream, j.pl, j.p, j.q,
                       j.rp + g.M + 1);
    IPD_KERNEL_CHECK();
    exclusive_scan_i32(ctx, j.pl.rowlen, j.rp, g.M);
    auto fill = [&](long long cap) {
        h->ci = j.dst.alloc<int>((size_t)cap);
        h->va = j.dst.alloc<double>((size_t)cap);
        if (cap == 0) return;
        hipLaunchKernelGGL(k_asat_fill, dim3(g.tiles_grid()), dim3(256), 0, ctx->stream, j.pl, j.p, j.q, j.rp,
                           h->ci, h->va, (int)cap);
        IPD_KERNEL_CHECK();
        // one wave per 64 rows (the sums are one dependent chain per row, so rows go to as many CUs as there
        // are: a 256-thread block per 256 rows left 248 CUs idle at m = n = 1024), both sides in one launch
        hipLaunchKernelGGL(k_asat_diag, dim3(g.diag_grid()), dim3(64), 0, ctx->stream, j.pl, j.p, j.q,
                           g.njb, j.rp, h->ci, h->va, (int)cap);
        IPD_KERNEL_CHECK();
    };
    const long long guess = asat_cap(ctx->asat_nnz_hint, g.m, g.n);
    if (guess > 0) fill(guess);
    int meta[2] = {0, 0};
    ctx->fetch(j.rp + g.M, meta, 2);
    h->nnz = meta[0];
    if (guess == 0 || !asat_accepts(h->nnz, guess)) fill(h->nnz);
    ctx->asat_nnz_hint = asat_hint_after_general(h->nnz);
    *zero_squares = meta[1] != 0;
}

// zero squares: drop the explicit zeros (MATLAB stores none)
static void asat_finish(ipd_ctx* ctx, Arena& dst, Csr h, bool zero_squares, Csr* H) {
    if (zero_squares && h.nnz) csr_drop_zeros(ctx, dst, Csr(h), &h);   // (reads its copy, then sets h)
    *H = h;
}

void kkt_asat(ipd_ctx* ctx, Arena& dst, const uint8_t* s, const double* p, const double* q, int m,
              int n, Csr* H) {
    kkt_require(asat_check_mn(m, n));
    const AsatGeo g = asat_geo(m, n);
    const AsatJob job{ctx, dst, g, asat_scratch(*ctx->scratch, g), p, q, dst.alloc<int>(g.rp_len())};
    unsigned ticket = 0;
    const bool small = asat_small_route(ctx->asat_nnz_hint, g) && ctx->mailbox_begin(&ticket);
    if (!small) job.clear_zflag();   // (k_asat_small writes the flag itself)
    const bool wide = asat_wide(m, reinterpret_cast<uintptr_t>(s));
    hipLaunchKernelGGL(wide ? k_asat_masks<true> : k_asat_masks<false>, dim3(g.tiles_grid()), dim3(256), 0, ctx->stream,
                       s, job.pl);
    IPD_KERNEL_CHECK();
    Csr h{g.M, g.M, 0, job.rp, nullptr, nullptr};
    bool zero_squares = false;
    if (!(small && asat_small(job, ticket, &h, &zero_squares))) asat_general(job, &h, &zero_squares);
    asat_finish(ctx, dst, h, zero_squares, H);
}

// ---------------------------------------------------------------------------
// C ABI (the frames: ipd_kkt.h)
// ---------------------------------------------------------------------------
extern "C" int ipd_asat_dev(ipd_ctx* ctx, const uint8_t* s, const double* p, const double* q,
                            int64_t m, int64_t n, ipd_dmat** H) {
    return kkt_dev_entry(ctx, s && p && q && H, m, n, [&](int mi, int ni) {
        std::unique_ptr<ipd_dmat> d(new ipd_dmat());
        d->ctx = ctx;
        d->arena.reset(new Arena(&ctx->pool));
        kkt_asat(ctx, *d->arena, s, p, q, mi, ni, &d->m);
        *H = d.release();
    });
}

extern "C" int ipd_asat(ipd_ctx* ctx, const uint8_t* s, const double* p, const double* q,
                        int64_t m, int64_t n, ipd_csc_out* H) {
    return kkt_host_entry(ctx, {{s, (size_t)m * (size_t)n}}, p, q, m, n, H, 0,
                          [&](const void* const* d, const double* dp, const double* dq, double*, int mi, int ni) {
                              Csr h;
                              kkt_asat(ctx, *ctx->scratch, static_cast<const uint8_t*>(d[0]), dp, dq, mi, ni, &h);
                              csr_download_as_csc(ctx, h, /*H symmetric: CSR == CSC*/ true, H);
                          });
}
