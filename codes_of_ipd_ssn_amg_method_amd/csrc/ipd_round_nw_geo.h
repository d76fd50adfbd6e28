// Geometry of the north-west-corner correction of ipd_round_nw.hip: the prefix buffer, the
// dense slots the merge writes, the list and the scratch a side takes, beside ipd_round_geo.h.  Host-clean: no HIP
// types, no getenv (the index functions are __host__ __device__ under hipcc only) -- the CPU test of this header
// (tests/round_nw_geo_driver.cpp) checks what the device runs.
//
//   prefixes   [C_0 .. C_n; R_0 .. R_m]: n + m + 2 doubles, C_s at nw_pre_col(s), R_k at nw_pre_row(n, k)
//   scan       chunks of NW_CHUNK entries; one thread per chunk of one workgroup, so a vector has at most
//              NW_THREADS chunks: m, n <= NW_CHUNK*NW_THREADS = 16384, the drivers' own limit
//   slots      entry (k, s), 1-based along the orders, has the dense slot (k - 1) + (s - 1): the entries form a
//              staircase, so the slots of two entries differ and ascend with (k, s); m + n - 1 slots
//   compaction thread t of the one workgroup owns the slots [t*span, (t + 1)*span) below the slot count
//   list       at most m + n - 1 entries; the workspace keeps m + n per side
#pragma once

#include <cstddef>
#include <cstdint>

#include "ipd_walk_geo.h"

constexpr int NW_CHUNK = 64;         // entries of a scan chunk
constexpr int NW_THREADS = 256;      // threads of every workgroup of the unit
constexpr int NW_MAX_LEN = NW_CHUNK * NW_THREADS;   // longest vector the one-workgroup scan takes
constexpr int NW_INFO_DOUBLES = 8;   // what the last kernel leaves for the read-back beside the statistics
constexpr int NW_SLOT_INTS = 2;      // (i, j) per dense slot
constexpr int NW_SLOT_DOUBLES = 3;   // (g, c*g, phi*g) per dense slot
constexpr int NW_LIST_DOUBLES = 2;   // (c*g, phi*g) per list entry, in list order
constexpr int NW_DEV_DOUBLES = 8;    // the scalars the writing pass reads (t = 0 there)

WK_HD_INLINE int nw_chunks(int len) { return (len + NW_CHUNK - 1) / NW_CHUNK; }
WK_HD_INLINE size_t nw_pre_len(int m, int n) { return (size_t)m + (size_t)n + 2; }
WK_HD_INLINE size_t nw_pre_col(int s) { return (size_t)s; }                           // s = 0 .. n
WK_HD_INLINE size_t nw_pre_row(int n, int k) { return (size_t)n + 1 + (size_t)k; }    // k = 0 .. m
WK_HD_INLINE int nw_slots(int m, int n) { return m + n - 1; }
WK_HD_INLINE int nw_slot(int k, int s) { return (k - 1) + (s - 1); }                  // k = 1 .. m, s = 1 .. n
WK_HD_INLINE int nw_span(int slots) { return (slots + NW_THREADS - 1) / NW_THREADS; }
WK_HD_INLINE size_t nw_list_cap(int m, int n) { return (size_t)m + (size_t)n; }

// bytes a side takes from the scratch arena on top of round_scratch_bytes (allocation granules aside)
static inline size_t round_nw_scratch_bytes(int m, int n) {
    const size_t M = nw_list_cap(m, n);
    return (nw_pre_len(m, n) + (NW_SLOT_DOUBLES + NW_LIST_DOUBLES) * M + NW_DEV_DOUBLES + NW_INFO_DOUBLES) *
               sizeof(double) +
           NW_SLOT_INTS * M * sizeof(int32_t);
}
// bytes the workspace keeps from the first ipd_apd_set_correction on: the two orders and a list per side
static inline size_t round_nw_workspace_bytes(int m, int n) {
    const size_t M = nw_list_cap(m, n);
    return M * sizeof(int32_t) + 2 * M * (2 * sizeof(int32_t) + sizeof(double));
}
