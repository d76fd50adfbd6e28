// The LDS images of the single-workgroup kernels and the polynomial operators: the kernels that pack them on the
// device, the host code that binds a planned layout (ipd_level_plan.h) to a descriptor and packs it, and the
// introspection entry points of what was packed.  The images' readers are ipd_small.hip's kernels and the resident
// kernels' tail workgroup; the row-layout operators' readers are the resident kernels.
#include "ipd_cycle_state.h"

struct PackEntry {
    const void* src;
    unsigned dst_off, bytes;  // multiples of 4
};
// compact copy of a block-wide polynomial operator (column-major, gld rows per column) with ld rows per column
// (SolveDesc::bm_src): one workgroup per column
// (the last workgroup copies the vector W behind the columns)
__global__ __launch_bounds__(128) void k_bm_compact(const double* __restrict__ src, int gld, double* __restrict__ dst,
                                                    int ld, const double* __restrict__ W, int rows) {
    const int c = blockIdx.x, r = threadIdx.x;
    if (c == (int)gridDim.x - 1) {
        if (r < ld) dst[(size_t)c * ld + r] = r < rows ? W[r] : 0.0;
        return;
    }
    if (r < ld) dst[(size_t)c * ld + r] = src[(size_t)c * gld + r];
}
// gathers the constant arrays of the cached levels into the image (one workgroup per array)
__global__ __launch_bounds__(256) void k_pack_image(const PackEntry* __restrict__ ents,
                                                    char* __restrict__ img) {
    const PackEntry e = ents[blockIdx.x];
    const int* src = reinterpret_cast<const int*>(e.src);
    int* dst = reinterpret_cast<int*>(img + e.dst_off);
    for (unsigned i = threadIdx.x; i < e.bytes / 4; i += 256) dst[i] = src[i];
}

struct DenseEntry {
    const int* rp;
    const int* ci;
    const double* va;
    int rows, cols;
    unsigned dst_off;
    int ld_row;   // 0: column-major; > 0: row-major with this leading dimension (dense thread-per-row levels)
};
// dense column-major copies of the tiny levels' operators (one workgroup per matrix)
__global__ __launch_bounds__(256) void k_pack_dense(const DenseEntry* __restrict__ ents,
                                                    char* __restrict__ img) {
    const DenseEntry e = ents[blockIdx.x];
    double* dst = reinterpret_cast<double*>(img + e.dst_off);
    const int total = e.ld_row ? e.rows * e.ld_row : e.rows * e.cols;
    for (int t = threadIdx.x; t < total; t += 256) dst[t] = 0.0;
    __syncthreads();
    for (int r = threadIdx.x; r < e.rows; r += 256)
        for (int t = e.rp[r]; t < e.rp[r + 1]; ++t) {
            if (e.ld_row) dst[(size_t)r * e.ld_row + e.ci[t]] = e.va[t];
            else dst[r + (size_t)e.ci[t] * e.rows] = e.va[t];
        }
}

// Lane map of a thread-per-row level (see blk_sweeps): one workgroup per level.
struct LmapEntry {
    const int* rp;
    int N;
    unsigned off;
};
__global__ __launch_bounds__(BT) void k_pack_lmap(const LmapEntry* __restrict__ ents, char* __restrict__ img) {
    __shared__ int wsum[BT / 64];
    __shared__ int cnt[5], base[5];
    const LmapEntry e = ents[blockIdx.x];
    unsigned* map = reinterpret_cast<unsigned*>(img + e.off);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int len = t < e.N ? e.rp[t + 1] - e.rp[t] : 0;
    auto block_sum = [&](int v) {
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        __syncthreads();
        if (lane == 0) wsum[wv] = v;
        __syncthreads();
        int s = 0;
        for (int w = 0; w < BT / 64; ++w) s += wsum[w];
        return s;
    };
    auto block_max = [&](int v) {
        for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
        __syncthreads();
        if (lane == 0) wsum[wv] = v;
        __syncthreads();
        int s = 0;
        for (int w = 0; w < BT / 64; ++w) s = max(s, wsum[w]);
        return s;
    };
    const int maxlen = block_max(len);
    int E = 2, need = 0;
    for (;; E <<= 1) {
        int n = 1;
        while (n < 16 && n * E < len) n <<= 1;
        need = t < e.N ? n : 0;
        if (block_sum(need) <= BT || E >= (1 << 20)) break;   // (uniform)
    }
    int lg = 0;
    while ((1 << lg) < need) ++lg;
    if (t < 5) cnt[t] = 0;
    map[t] = 0u;
    __syncthreads();
    // rank of the row among the rows of its class, in row order
    int rank = 0;
    for (int c = 0; c < 5; ++c) {
        const bool mine = t < e.N && lg == c;
        const unsigned long long b = __ballot(mine);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        __syncthreads();
        if (lane == 0) wsum[wv] = __popcll(b);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < BT / 64; ++w) {
            if (w < wv) woff += wsum[w];
            tot += wsum[w];
        }
        if (mine) rank = woff + before;
        if (t == 0) cnt[c] = tot;
    }
    __syncthreads();
    if (t == 0) {   // classes by descending group size: every group is aligned to its size
        int off = 0;
        for (int c = 4; c >= 0; --c) {
            base[c] = off;
            off += cnt[c] << c;
        }
        map[BT] = (E <= 16 && maxlen <= 16 * E) ? (unsigned)E : 0u;
    }
    __syncthreads();
    if (t < e.N) {
        const int b0 = base[lg] + (rank << lg);
        for (int s = 0; s < (1 << lg); ++s)
            map[b0 + s] = (unsigned)t | ((unsigned)s << 10) | ((unsigned)lg << 14) | (1u << 31);
    }
}

// Polynomial form of a one-wave level (see poly_pre / poly_post): one workgroup per level forms
//   Rg = R + u 1', u = (1 - R A1) / xx (isnsp) or 0 ;  S = I - Rg A ;  M1 = S^nu ;
//   M2 = sum_{j<nu} S^j Rg = M2a + w 1'  with  M2a = sum S^j R ,  w = sum S^j u
//   T1 = P'A ;  Mr = [M2a; P' - T1 M2a] ;  W = [w; -T1 w] ;  Me = [M1; -T1 M1] ;  Mc = M1 P
// with dense column-major matrices in LDS and writes Mr, Me, Mc, W into the image.  The rank-one part
// w 1' stays apart because u ~ 1/xx is large (xx = 1'A1 ~ N bk1): added into every entry of M2 it
// would cost the cancellation inside 1'r that the sweeps' own xig = 1'g enjoys (MG_Vcycle.m:17).
struct PolyEntry {
    const int *Arp, *Aci;
    const double* Ava;
    const int *Prp, *Pci;   // P  : N x Nc  (CSR)
    const double* Pva;
    const double* dinv;
    const double* Axi;
    const double* xx;
    int N, Nc, nu, isnsp, LD;
    unsigned offMr, offMe, offMc, offW;
};
__global__ __launch_bounds__(BT) void k_pack_poly(const PolyEntry* __restrict__ ents, char* __restrict__ img) {
    extern __shared__ __attribute__((aligned(16))) char poly_raw[];
    const PolyEntry e = ents[blockIdx.x];
    const int N = e.N, Nc = e.Nc, R = N + Nc, LD = e.LD, t = threadIdx.x;
    const int N8 = (N + 7) / 8 * 8, Nc8 = (Nc + 7) / 8 * 8;
    double* A = reinterpret_cast<double*>(poly_raw);   // N x N, column-major like everything here
    double* S = A + N * N;
    double* M1 = S + N * N;
    double* M2 = M1 + N * N;                            // M2a
    double* T = M2 + N * N;                             // product scratch
    double* P = T + N * N;                              // N x Nc
    double* T1 = P + N * Nc;                            // Nc x N
    double* u = T1 + Nc * N;                            // N
    double* dv = u + N;                                 // N
    double* w = dv + N;                                 // N
    double* w2 = w + N;                                 // N
    for (int i = t; i < N * N; i += BT) A[i] = 0.0;
    for (int i = t; i < N * Nc; i += BT) P[i] = 0.0;
    __syncthreads();
    for (int r = t; r < N; r += BT) {
        for (int q = e.Arp[r]; q < e.Arp[r + 1]; ++q) A[r + e.Aci[q] * N] = e.Ava[q];
        for (int q = e.Prp[r]; q < e.Prp[r + 1]; ++q) P[r + e.Pci[q] * N] = e.Pva[q];
        const double d = e.dinv[r];
        dv[r] = d;
        u[r] = e.isnsp ? (1.0 - d * e.Axi[r]) / e.xx[0] : 0.0;
        w[r] = 0.0;
    }
    __syncthreads();
    // S = I - Rg A,  (Rg A)[i][j] = dinv_i A[i][j] + u_i (1'A)_j ;  M1 = I ;  M2a = 0 ;  w = 0
    for (int q = t; q < N * N; q += BT) {
        const int i = q % N, j = q / N;
        double cs = 0.0;
        for (int k = 0; k < N; ++k) cs += A[k + j * N];
        S[q] = (i == j ? 1.0 : 0.0) - (dv[i] * A[q] + u[i] * cs);
        M1[q] = i == j ? 1.0 : 0.0;
        M2[q] = 0.0;
    }
    __syncthreads();
    for (int s = 0; s < e.nu; ++s) {
        // M2a <- R + S M2a ;  w <- u + S w ;  M1 <- S M1     (results parked: all read the old values)
        for (int q = t; q < 2 * N * N + N; q += BT) {
            if (q >= 2 * N * N) {
                const int i = q - 2 * N * N;
                double acc = 0.0;
                for (int k = 0; k < N; ++k) acc += S[i + k * N] * w[k];
                w2[i] = u[i] + acc;
                continue;
            }
            const bool second = q >= N * N;
            const int qq = second ? q - N * N : q;
            const int i = qq % N, j = qq / N;
            const double* B = second ? M1 : M2;
            double acc = 0.0;
            for (int k = 0; k < N; ++k) acc += S[i + k * N] * B[k + j * N];
            if (second)
                T[qq] = acc;
            else
                A[qq] = acc + (i == j ? dv[i] : 0.0);   // A is rebuilt below; until then: second scratch
        }
        __syncthreads();
        for (int q = t; q < N * N; q += BT) {
            M1[q] = T[q];
            M2[q] = A[q];
        }
        for (int i = t; i < N; i += BT) w[i] = w2[i];
        __syncthreads();
    }
    // A again (it was scratch), then T1 = P'A
    for (int i = t; i < N * N; i += BT) A[i] = 0.0;
    __syncthreads();
    for (int r = t; r < N; r += BT)
        for (int q = e.Arp[r]; q < e.Arp[r + 1]; ++q) A[r + e.Aci[q] * N] = e.Ava[q];
    __syncthreads();
    for (int q = t; q < Nc * N; q += BT) {
        const int c = q % Nc, j = q / Nc;
        double acc = 0.0;
        for (int k = 0; k < N; ++k) acc += P[k + c * N] * A[k + j * N];
        T1[q] = acc;
    }
    __syncthreads();
    double* Mr = reinterpret_cast<double*>(img + e.offMr);
    double* Me = reinterpret_cast<double*>(img + e.offMe);
    double* Mc = reinterpret_cast<double*>(img + e.offMc);
    double* W = reinterpret_cast<double*>(img + e.offW);
    for (int q = t; q < LD * N8; q += BT) {
        const int row = q % LD, j = q / LD;
        double vr = 0.0, ve = 0.0;
        if (j < N && row < N) {
            vr = M2[row + j * N];
            ve = M1[row + j * N];
        } else if (j < N && row < R) {
            const int c = row - N;
            double a2 = 0.0, a1 = 0.0;
            for (int k = 0; k < N; ++k) {
                a2 += T1[c + k * Nc] * M2[k + j * N];
                a1 += T1[c + k * Nc] * M1[k + j * N];
            }
            vr = P[j + c * N] - a2;
            ve = -a1;
        }
        Mr[q] = vr;
        Me[q] = ve;
    }
    for (int q = t; q < LD * Nc8; q += BT) {
        const int i = q % LD, c = q / LD;
        double acc = 0.0;
        if (i < N && c < Nc)
            for (int k = 0; k < N; ++k) acc += M1[i + k * N] * P[k + c * N];
        Mc[q] = acc;
    }
    for (int row = t; row < LD; row += BT) {
        double v = 0.0;
        if (row < N) {
            v = w[row];
        } else if (row < R) {
            const int c = row - N;
            for (int k = 0; k < N; ++k) v += T1[c + k * Nc] * w[k];
            v = -v;
        }
        W[row] = v;
    }
}

// Block-wide polynomial form of a 33..144-row level (SolveLevel::gM): the recurrences of k_pack_poly
// as dense products on the f64 matrix cores.  All operands live in global scratch, column-major, padded
// with zeros to multiples of 16 (Np rows; no edge cases in the tiles).  M1 = S^nu by nu - 1 products
// S^j = S S^(j-1); their running sum I + S + ... + S^(nu-1) gives M2a (columns scaled by D^-1) and w
// (applied to u).  Y = [sum | S^nu | w, 15 zero columns] is one matrix of 2 Np + 16 columns, so that the
// rows below N of the output are one more product, T1 Y.  One wave per 16 x 16 tile
// (v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; result
// register g of lane l is C[(l >> 4) + 4 g][l & 15]), the operand loads of 64 k in flight.
struct BPolyEntry {
    const int* Arp;
    const int* Aci;
    const double* Ava;
    const int* Prp;
    const int* Pci;
    const double* Pva;
    const double* dinv;
    const double* Axi;
    const double* xx;
    int N, Nc, Np, Ncp, nu, isnsp, LD;
    double* A;    // Np x Np
    double* S;    // Np x Np
    double* P;    // Np x Ncp
    double* T1;   // Ncp x Np = P'A
    double* Pw[2]; // Np x Np: the powers of S, ping-pong
    double* Y;     // Np x (2 Np + 16): [I + S + ... + S^(nu-1) | S^nu | w, 15 zero columns]
    double* dv;
    double* u;
    double* cs;   // column sums of A
    double* M;    // out: [Mr | Me | Mc], LD rows, 8-padded column counts (zeroed by the host)
    double* W;    // out: LD
    // out, instead of M: row-major [N + Nc][RES_P3_LD] with Mr in columns 0..N-1, Me in 512..512+N-1
    // and Mc in 1024..1024+Nc-1 (the resident kernels' third level: a thread holds entries t, 512 + t
    // and 1024 + t of its workgroup's rows, ipd_resident.h POLY3); W then has N + Nc entries
    double* rows;
    int rows_seg;   // segment length of that layout: 512 (k_resident, Mc at most 128 columns) or RB_P3_SEG
    int rows_ld;    // its row stride
};
typedef double bp_d4 __attribute__((ext_vector_type(4)));
// (the k index of MFMA u in a group of four is k0 + 4 (l >> 4) + u, not k0 + 4 u + (l >> 4): a lane's four
// B values are then 32 contiguous bytes and the four lanes of a column share one 128-byte line -- with
// the natural order every load touched sixteen lines for 32 bytes each and a product of 288^3 took 14 us)
// One tile per WORKGROUP: wave w takes the 16-k groups w, w + 4, ... (a product is a chain of dependent
// batches of loads otherwise: 288 / 64 = 5 round trips to L2), the four partial tiles are added in wave
// order through LDS; the sum is returned to wave 0 only.
__device__ __forceinline__ bp_d4 bp_tile(const double* __restrict__ A, int a_is, int a_ks,
                                         const double* __restrict__ B, int b_ks, int b_js, int K, int I0, int J0) {
    typedef double bp_v2 __attribute__((ext_vector_type(2)));
    __shared__ double bp_part[3][4][64];
    const int l = threadIdx.x & 63, r = l & 15, q = l >> 4, wv = threadIdx.x >> 6;
    const double* ap = A + (size_t)(I0 + r) * a_is + (size_t)(4 * q) * a_ks;
    const double* bp = B + (size_t)(4 * q) * b_ks + (size_t)(J0 + r) * b_js;   // b_ks == 1
    bp_d4 c = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < K; k0 += 256) {
        double a[16], b[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int k = k0 + 16 * (4 * g + wv);
            const bool in = k < K;   // uniform (K is a multiple of 16)
            if (in) {
                const bp_v2 b01 = *reinterpret_cast<const bp_v2*>(bp + k);
                const bp_v2 b23 = *reinterpret_cast<const bp_v2*>(bp + k + 2);
                b[4 * g] = b01.x;
                b[4 * g + 1] = b01.y;
                b[4 * g + 2] = b23.x;
                b[4 * g + 3] = b23.y;
                if (a_ks == 1) {
                    const bp_v2 a01 = *reinterpret_cast<const bp_v2*>(ap + k);
                    const bp_v2 a23 = *reinterpret_cast<const bp_v2*>(ap + k + 2);
                    a[4 * g] = a01.x;
                    a[4 * g + 1] = a01.y;
                    a[4 * g + 2] = a23.x;
                    a[4 * g + 3] = a23.y;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[4 * g + u] = ap[(size_t)(k + u) * a_ks];
                }
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) a[4 * g + u] = b[4 * g + u] = 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (k0 + 16 * (4 * (u / 4) + wv) < K) c = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], c, 0, 0, 0);
    }
    if (wv > 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) bp_part[wv - 1][g][l] = c[g];
    }
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int ww = 0; ww < 3; ++ww)
#pragma unroll
            for (int g = 0; g < 4; ++g) c[g] += bp_part[ww][g][l];
    }
    return c;
}
// dense copies of A and P, D^-1, u, and the parts of the state after the first sweep that are not S:
// M2a = D^-1, w = u
__global__ __launch_bounds__(256) void k_bpoly_scatter(const BPolyEntry e) {   // one wave per row
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, Np = e.Np;
    if (r >= e.N) return;
    for (int q = e.Arp[r] + lane; q < e.Arp[r + 1]; q += 64) e.A[r + (size_t)e.Aci[q] * Np] = e.Ava[q];
    for (int q = e.Prp[r] + lane; q < e.Prp[r + 1]; q += 64) e.P[r + (size_t)e.Pci[q] * Np] = e.Pva[q];
    if (lane == 0) {
        const double d = e.dinv[r];
        const double ui = e.isnsp ? (1.0 - d * e.Axi[r]) / e.xx[0] : 0.0;
        e.dv[r] = d;
        e.u[r] = ui;
        if (e.nu == 1) e.Y[r + (size_t)(2 * Np) * Np] = ui;   // w = u
    }
}
__global__ __launch_bounds__(256) void k_bpoly_colsum(const BPolyEntry e) {   // one wave per column
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= e.N) return;
    const double* aj = e.A + (size_t)j * e.Np;
    double cs = 0.0;
    for (int k = lane; k < e.N; k += 64) cs += aj[k];
    cs = wave_sum(cs);
    if (lane == 0) e.cs[j] = cs;
}
// S = I - Rg A with (Rg A)[i][j] = dinv_i A[i][j] + u_i (1'A)_j, the first power and the sum so far
// (blocks below nS: one thread per entry); T1 = P'A (the tiles behind)
__global__ __launch_bounds__(256) void k_bpoly_S_T1(const BPolyEntry e, int nS) {
    const int N = e.N, Np = e.Np;
    if ((int)blockIdx.x < nS) {
        const int q = blockIdx.x * 256 + threadIdx.x;
        if (q >= N * N) return;
        const int i = q % N, j = q / N;
        const size_t at = i + (size_t)j * Np;
        const double id = i == j ? 1.0 : 0.0;
        const double sv = id - (e.dv[i] * e.A[at] + e.u[i] * e.cs[j]);
        e.S[at] = sv;
        e.Pw[0][at] = sv;
        e.Y[at] = e.nu >= 2 ? id + sv : id;
        if (e.nu == 1) e.Y[at + (size_t)Np * Np] = sv;
        return;
    }
    const int tile = (int)blockIdx.x - nS, ni = e.Ncp / 16;
    const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni), l = threadIdx.x & 63;
    const bp_d4 c = bp_tile(e.P, Np, 1, e.A, 1, Np, Np, I0, J0);   // A-operand (c, k) = P[k + c Np]
    if (threadIdx.x >= 64) return;
    for (int g = 0; g < 4; ++g) e.T1[(I0 + (l >> 4) + 4 * g) + (size_t)(J0 + (l & 15)) * e.Ncp] = c[g];
}
// S^s = S S^(s-1) (s = 2 .. nu; the last one lands in Y's second block), added to the sum while s < nu;
// beside the last product: w = (I + ... + S^(nu-1)) u, one wave per row
__global__ __launch_bounds__(256) void k_bpoly_step(const BPolyEntry e, int s, int src, int nT) {
    const int Np = e.Np, ni = Np / 16, l = threadIdx.x & 63;
    if ((int)blockIdx.x >= nT) {
        const int i = ((int)blockIdx.x - nT) * 4 + (threadIdx.x >> 6);
        if (i >= e.N) return;
        double acc = 0.0;
        for (int j = l; j < e.N; j += 64) acc += e.Y[i + (size_t)j * Np] * e.u[j];
        acc = wave_sum(acc);
        if (l == 0) e.Y[i + (size_t)(2 * Np) * Np] = acc;
        return;
    }
    const int tile = blockIdx.x;
    const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
    const bp_d4 c = bp_tile(e.S, 1, Np, e.Pw[src], 1, Np, Np, I0, J0);
    if (threadIdx.x >= 64) return;
    double* dst = s == e.nu ? e.Y + (size_t)Np * Np : e.Pw[src ^ 1];
    const int j = J0 + (l & 15);
    for (int g = 0; g < 4; ++g) {
        const size_t at = (size_t)(I0 + (l >> 4) + 4 * g) + (size_t)j * Np;
        dst[at] = c[g];
        if (s < e.nu) e.Y[at] += c[g];
    }
}
// the stacked output: rows below N from -T1 Y (+ P' in the Mr block), Mc = M1 P, copies above
__global__ __launch_bounds__(256) void k_bpoly_final(const BPolyEntry e, int nZ, int nC) {
    const int N = e.N, Nc = e.Nc, Np = e.Np, Ncp = e.Ncp, LD = e.LD, l = threadIdx.x & 63;
    const int N8 = (N + 7) / 8 * 8;
    const double* Y = e.Y;
    auto put = [&](int row, bool me, int j, double v) {
        if (e.rows)
            e.rows[(size_t)row * e.rows_ld + (me ? e.rows_seg : 0) + j] = v;
        else
            e.M[row + (size_t)((me ? N8 : 0) + j) * LD] = v;
    };
    int blk = blockIdx.x;
    if (blk < nZ) {   // Z = T1 Y: Ncp x (2 Np + 16)
        const int ni = Ncp / 16, tile = blk;
        const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
        const bp_d4 c = bp_tile(e.T1, 1, Ncp, Y, 1, Np, Np, I0, J0);
        if (threadIdx.x >= 64) return;
        const int j = J0 + (l & 15);
        for (int g = 0; g < 4; ++g) {
            const int cc = I0 + (l >> 4) + 4 * g;
            if (cc >= Nc) continue;
            if (j < Np) {
                if (j < N) put(N + cc, false, j, e.P[j + (size_t)cc * Np] - c[g] * e.dv[j]);
            } else if (j < 2 * Np) {
                if (j - Np < N) put(N + cc, true, j - Np, -c[g]);
            } else if (j == 2 * Np) {
                e.W[N + cc] = -c[g];
            }
        }
        return;
    }
    blk -= nZ;
    if (blk < nC) {   // Mc = M1 P: Np x Ncp
        const int ni = Np / 16, tile = blk;
        const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
        const bp_d4 c = bp_tile(Y + (size_t)Np * Np, 1, Np, e.P, 1, Np, Np, I0, J0);
        if (threadIdx.x >= 64) return;
        const int j = J0 + (l & 15);
        for (int g = 0; g < 4; ++g) {
            const int i = I0 + (l >> 4) + 4 * g;
            if (i < N && j < Nc) {
                if (e.rows)
                    e.rows[(size_t)i * e.rows_ld + 2 * e.rows_seg + j] = c[g];
                else
                    e.M[i + (size_t)(2 * N8 + j) * LD] = c[g];
            }
        }
        return;
    }
    blk -= nC;
    const int q = blk * 256 + threadIdx.x;   // copies: M2a = sum D^-1, M1, w
    if (q < N * N) {
        const int i = q % N, j = q / N;
        put(i, false, j, Y[i + (size_t)j * Np] * e.dv[j]);
        put(i, true, j, Y[i + (size_t)(Np + j) * Np]);
    } else if (q < N * N + N) {
        const int i = q - N * N;
        e.W[i] = Y[i + (size_t)(2 * Np) * Np];
    }
}

// Level 2 of the resident kernel, composed over a whole visit (ResDesc::p2rows; pack_bpoly in its row layout
// has run): B = M1 M2a + M2a into the Me segment of the rows (tiles below nT), wB = M1 w + w into W (one wave
// per row behind).  M1 = Y's second block, M2a = Y's first block with columns scaled by D^-1, w = Y's column 2 Np.
__global__ __launch_bounds__(256) void k_bpoly_compose(const BPolyEntry e, int nT) {
    const int N = e.N, Np = e.Np, l = threadIdx.x & 63;
    const double* Y = e.Y;
    if ((int)blockIdx.x >= nT) {
        const int i = ((int)blockIdx.x - nT) * 4 + (threadIdx.x >> 6);
        if (i >= N) return;
        double acc = 0.0;
        for (int j = l; j < N; j += 64) acc += Y[i + (size_t)(Np + j) * Np] * Y[j + (size_t)(2 * Np) * Np];
        acc = wave_sum(acc);
        if (l == 0) e.W[i] = acc + Y[i + (size_t)(2 * Np) * Np];
        return;
    }
    const int ni = Np / 16, tile = blockIdx.x;
    const int I0 = 16 * (tile % ni), J0 = 16 * (tile / ni);
    const bp_d4 c = bp_tile(Y + (size_t)Np * Np, 1, Np, Y, 1, Np, Np, I0, J0);
    if (threadIdx.x >= 64) return;
    const int j = J0 + (l & 15);
    for (int g = 0; g < 4; ++g) {
        const int i = I0 + (l >> 4) + 4 * g;
        if (i < N && j < N)
            e.rows[(size_t)i * e.rows_ld + e.rows_seg + j] = (c[g] + Y[i + (size_t)j * Np]) * e.dv[j];
    }
}

// Packs the polynomial form of level k (k_bpoly_*) into the hierarchy's arena, in the layout asked for
// (ipd_cycle_state.h)
BPolyPack pack_bpoly(ipd_ctx* ctx, ipd_amg* h, CycleState* st, int k, int isnsp, int LD, bool rows, int rows_seg,
                     int rows_ld) {
    Arena& ar = *h->arena;
    BPolyPack b;
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
    b.ops = std::make_shared<const BPolyEntry>(e);
    return b;
}

// what a row-layout pack holds (its own layout), for ipd_amg_packed_operator
CycleState::RowsOp rows_op(const BPolyPack& b) {
    CycleState::RowsOp r;
    r.M = b.M;
    r.ld = b.ops->rows_ld;
    r.seg = b.ops->rows_seg;
    r.N = b.ops->N;
    r.Nc = b.ops->Nc;
    return r;
}
// one kernel's set of row-layout levels: level 3 is packed first and starts the set afresh, so that a
// hierarchy planned for one resident kernel and then for another never reports a mix of the two
void record_rows_op(CycleState* st, const ipd_amg* h, int k, const BPolyPack& b) {
    if (k == 3) st->rows_ops.assign((size_t)h->J + 1, CycleState::RowsOp{});
    st->rows_ops.resize((size_t)h->J + 1);
    st->rows_ops[(size_t)k] = rows_op(b);
}

// level 2 of the resident kernel composed over a whole visit, on a row-layout pack of it (ipd_cycle_state.h)
void bpoly_compose(ipd_ctx* ctx, const BPolyPack& b) {
    const BPolyEntry& e = *b.ops;
    const int nT = (e.Np / 16) * (e.Np / 16);
    // (IPD_OPTIN_LDS is not needed: the tiles use static LDS only)
    hipLaunchKernelGGL(k_bpoly_compose, dim3((unsigned)(nT + (e.N + 3) / 4)), dim3(256), 0, ctx->stream, e, nT);
    IPD_KERNEL_CHECK();
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
            const int LD = (int)own.ld();
            const BPolyPack b = pack_bpoly(ctx, h, st, k, sd->isnsp, LD, false, 0, 0);   // (no row layout)
            po = CycleState::PolyOp{b.M, b.W, LD, h->L[k].A.nr, h->L[k + 1].A.nr};
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
// by its role (ipd_cycle_state.h)
void pack_image(ipd_ctx* ctx, ipd_amg* h, CycleState* st, const std::vector<LevelShape>& shapes, const LevelPlan& plan,
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
