// Host rules of the KKT operators Ax, Aty, ASAt, invAAt and invHHt (ipd_kkt.hip, ipd_asat.hip), each written once:
// the dimension checks, the grids and scratch sizes, ASAt's route between its one-launch and its general assembly
// with the capacity guess, the accept test and the hint update, and the alignment predicates that choose a kernel
// form.  The executors call these and compare no size against a threshold.  Host-clean, no HIP, no getenv:
// tests/kkt_plan_driver.cpp runs it on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "ipd_amg.h"      // IPD_OK, IPD_E_ARG, IPD_E_LIMIT
#include "ipd_limits.h"

static constexpr int kkt_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- dimension checks: the error kind and its message; the caller throws ------------------------
struct KktDimCheck {
    int code;          // IPD_OK, or the error the entry reports
    const char* msg;
};
// every entry of the C ABI
static inline KktDimCheck kkt_check_mn(int64_t m, int64_t n) {
    if (!(m > 0 && n > 0)) return {IPD_E_ARG, "m and n must be positive"};
    if (!(m < (1 << 28) && n < (1 << 28) && m * n < (int64_t(1) << 40))) return {IPD_E_LIMIT, "m*n too large"};
    return {IPD_OK, nullptr};
}
// H has at most 2*m*n + m + n entries and its row pointers, entry counts and tile counts are 32-bit: ASAt refuses
// what could wrap (e.g. m = n = 40000 at rho ~ 1 fits in HBM but not in int32)
static inline long long asat_worst_nnz(long long m, long long n) { return 2 * m * n + m + n; }
static inline KktDimCheck asat_check_mn(int m, int n) {
    if (!(m > 0 && n > 0)) return {IPD_E_ARG, "ASAt: empty p or q"};
    if (!(asat_worst_nnz(m, n) < (1LL << 31) - 64))
        return {IPD_E_LIMIT, "ASAt: 2*m*n + m + n must stay below 2^31 (32-bit row pointers)"};
    return {IPD_OK, nullptr};
}

// ---- Ax, Aty, invHHt ------------------------------------------------------------------------------
// Known limit: ax_geo().njb and aty_grid_y() = cdiv(n, 16) are a grid's y dimension, which takes far less than
// the n < 2^28 that kkt_check_mn admits ("KKT plan").
struct AxGeo {
    int nib, njb, final_grid;   // k_ax_tiles: tiles of AX_TR rows x AX_TC columns; k_ax_final: 256 entries of y each
    size_t lpart, rpart;        // partial row sums [njb][m], partial column sums [nib][n]
};
static inline AxGeo ax_geo(int m, int n) {
    const int nib = kkt_cdiv(m, AX_TR), njb = kkt_cdiv(n, AX_TC);
    return {nib, njb, kkt_cdiv((long long)m + n, 256), (size_t)njb * m, (size_t)nib * n};
}

// k_aty_v2 (two rows per lane, 16-byte stores) needs an even m and a 16-byte aligned z
static inline bool aty_vec2(int m, uintptr_t z_address) { return m % 2 == 0 && (z_address & 15) == 0; }
static inline int aty_grid_x(int m, bool vec2) { return kkt_cdiv(vec2 ? m / 2 : m, 256); }
static inline int aty_grid_y(int n) { return kkt_cdiv(n, ATY_TC); }

// partial sums of |phi|^2 (workgroups of k_sumsq_partial)
static inline int phi_parts(int m, int n) {
    return (int)std::max<size_t>(1, std::min<size_t>(((size_t)m * n + 255) / 256, PHI_PARTS_MAX));
}

// ---- ASAt -------------------------------------------------------------------------------------------
struct AsatGeo {
    int m, n;
    int nib, njb;      // mask tiles per column / per row
    int M;             // rows of H
    int ntiles;
    // scratch elements, in allocation order: colmask, rowmask (64-bit words), coloff, rowoff, cntc, cntr, rowlen
    size_t col_words() const { return (size_t)nib * n; }   // colmask, coloff
    size_t row_words() const { return (size_t)njb * m; }   // rowmask, rowoff
    size_t rp_len() const { return (size_t)M + 2; }        // rp[M] = nnz, rp[M+1] = zero-square flag
    // grids: masks and fill (a wave per tile, four per workgroup), offsets and small (a thread per row of H, 256 per
    // workgroup), diag (a wave per 64 rows: njb = cdiv(n,64) workgroups for the rows [0,n), then nib = cdiv(m,64))
    int tiles_grid() const { return kkt_cdiv(ntiles, 4); }
    int rows_grid() const { return kkt_cdiv(M, 256); }
    int diag_grid() const { return njb + nib; }
    size_t small_lds() const { return sizeof(double) * (size_t)M; }   // k_asat_small: p, then q
};
static inline AsatGeo asat_geo(int m, int n) {
    const int nib = kkt_cdiv(m, ASAT_TILE), njb = kkt_cdiv(n, ASAT_TILE);
    return {m, n, nib, njb, m + n, nib * njb};
}

// k_asat_masks<WIDE> reads a tile's column as eight 8-byte words
static inline bool asat_wide(int m, uintptr_t s_address) { return m % 8 == 0 && (s_address & 7) == 0; }

// entries ci/va are sized for before the count is known: the previous call's count + 25 % + 64, at most the worst
// case; 0 without a previous count
static inline long long asat_cap(long long hint, int m, int n) {
    return hint > 0 ? std::min(asat_worst_nnz(m, n), hint + hint / 4 + 64) : 0;
}
static inline bool asat_accepts(long long nnz, long long cap) { return nnz <= cap; }

// The one-launch route: a small previous count, and a row's masks in ASAT_SMALL_WORDS words on either side.  That
// bounds the workgroups of 256 rows by what one look-back sweep reads:
static_assert(kkt_cdiv(2LL * ASAT_SMALL_WORDS * ASAT_TILE, 256) <= ASAT_SMALL_WGS,
              "k_asat_small: one lane per predecessor workgroup");
static inline bool asat_small_route(long long hint, const AsatGeo& g) {
    return hint > 0 && hint <= ASAT_SMALL_HINT_MAX && g.nib <= ASAT_SMALL_WORDS && g.njb <= ASAT_SMALL_WORDS;
}
// the hint after a route's count: a give-up of the one-launch route leaves it alone, the general route always sets it
static inline long long asat_hint_after_small(long long hint, int nnz) { return nnz == ASAT_GAVE_UP ? hint : nnz; }
static inline long long asat_hint_after_general(int nnz) { return nnz; }
