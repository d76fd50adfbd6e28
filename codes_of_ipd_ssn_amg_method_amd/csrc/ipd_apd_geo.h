// Launch geometry of the drivers' tile walker (k_tiles, ipd_apd_tiles.h) and the sizes of the partial-sum buffers
// that follow from it.  x(i,j) = x[i + j*m]; a workgroup is 4 waves of 64 consecutive rows each (TR rows), a wave
// walks reps chunks of TC columns alone; the grid is nib x njg.  The walk itself: chunk `rep` of column group `jg`
// starts at column apd_step_col(g, jg, rep) and ends the walk when that is >= n.  Host-clean: no HIP types, no
// getenv -- the CPU test of this header (tests/apd_geo_driver.cpp) checks what the device runs.
#pragma once

#include <cstddef>
#include <cstring>

constexpr int TR = 256;        // tile rows
constexpr int TC = 16;         // tile columns per sub-tile
constexpr int APD_WAVES = 4;   // waves of a workgroup: one row of rpart per wave
constexpr int APD_REPS_MAX = 8;

struct Geo {
    int m, n, nib, njg, reps;  // njg column groups of reps*TC columns
};

static inline int apd_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// The value of IPD_APD_REPS (nullptr: unset): 0 = the natural rule, 1|2|4|8 = that many chunks per wave,
// -1 = anything else (the caller refuses it).
static inline int apd_reps_switch(const char* value) {
    if (!value || !value[0]) return 0;
    for (int r = 1; r <= APD_REPS_MAX; r *= 2) {
        const char want[2] = {(char)('0' + r), 0};
        if (!std::strcmp(value, want)) return r;
    }
    return -1;
}

// forced_reps = 0: a wave walks more columns once the grid is large anyway (from 4096 workgroups on)
static inline Geo make_geo(int m, int n, int forced_reps = 0) {
    Geo g;
    g.m = m;
    g.n = n;
    g.nib = apd_cdiv(m, TR);
    const int njb = apd_cdiv(n, TC);
    int reps = 1;
    if (forced_reps > 0)
        reps = forced_reps;
    else
        while (reps < APD_REPS_MAX && (long long)g.nib * apd_cdiv(njb, reps * 2) >= 4096) reps *= 2;
    g.reps = reps;
    g.njg = apd_cdiv(njb, reps);
    return g;
}

// first column of chunk `rep` of column group `jg`; the chunk owns columns [j0, j0 + TC) below n
static inline int apd_step_col(const Geo& g, int jg, int rep) { return (jg * g.reps + rep) * TC; }

// what a workspace allocates for the partial sums (apd_create_common)
static inline size_t apd_nblk(const Geo& g) { return (size_t)g.nib * g.njg; }                   // spart: NSC each
static inline size_t apd_lpart_len(const Geo& g) { return (size_t)g.njg * g.m; }                // row sums per column group
static inline size_t apd_rpart_len(const Geo& g) { return (size_t)g.nib * APD_WAVES * g.n; }    // column sums per wave
