// Every IPD_* environment switch the library reads, with the reason it stays (none is needed in
// production), and the two accessors all reads go through.  A switch is read where it takes effect
// (per hierarchy, per attach or per solve), never cached at load: the tests change the environment
// between calls in one process.
#pragma once

#include <cassert>
#include <cstdlib>
#include <cstring>

enum SwitchKind { SW_FLAG, SW_VALUE };   // flag: on when its value starts with '1'; value: read as is
struct SwitchInfo {
    const char* name;
    SwitchKind kind;
    const char* why;
};

static constexpr SwitchInfo IPD_SWITCHES[] = {
    {"IPD_NO_RESIDENT", SW_FLAG, "the multi-launch path as a whole: the reference point of every resident mode's tests"},
    {"IPD_NO_RESIDENT_REMOTE", SW_FLAG, "k_resident without its remote tail workgroup, against the launches (tests)"},
    {"IPD_NO_RESIDENT_THREE", SW_FLAG, "k_resident without level 3 in its workgroups, against the two-level form (tests)"},
    {"IPD_NO_RESIDENT_BIG", SW_FLAG, "the mask-form resident kernel off (tests)"},
    {"IPD_RESIDENT_BIG", SW_FLAG, "the mask-form resident kernel forced on sizes the oracle solves in seconds (tests)"},
    {"IPD_NO_RESIDENT_DEEP", SW_FLAG, "the mask-form kernel's deep mode off (tests: against the launches)"},
    {"IPD_NO_RES_POLY4", SW_FLAG, "deep mode / POLY3 mode with the tail rooted at level 4 (A/B of POLY4)"},
    {"IPD_RESIDENT_G", SW_VALUE, "<grid>: more resident workgroups than the rows need (measurement)"},
    {"IPD_RESIDENT_RANKS", SW_VALUE, "<R>: rank groups with a granule buffer each (the sharded resident kernel in emulation, tests)"},
    {"IPD_RES_PRESLEEP", SW_VALUE, "<n>: k_resident's s_sleep(1) count between a publish and the first poll (measurement)"},
    {"IPD_RES_DEBUG_SKIP_PUBLISH", SW_VALUE, "<step>: one omitted publish exercises the give-up and recovery path (tests)"},
    {"IPD_RES_NO_FULL", SW_FLAG, "k_resident's general form where the full-shape one applies: its bit-for-bit reference (tests) and A/B control"},
    {"IPD_NO_SUBCYCLE", SW_FLAG, "the single-workgroup sub-cycle off: the generic phases stay tested"},
    {"IPD_NO_SMALL", SW_FLAG, "the single-workgroup whole solve off: the generic phases stay tested"},
    {"IPD_NO_BLK", SW_FLAG, "the thread-per-row levels of the single-workgroup kernels off: their generic phases stay tested"},
    {"IPD_NO_POLY", SW_FLAG, "polynomial forms of the tail's levels off: the sweep forms stay tested against the oracle"},
    {"IPD_NO_BPOLY", SW_FLAG, "block-wide polynomial form off: the sweep forms stay tested against the oracle"},
    {"IPD_NO_BLKDENSE", SW_FLAG, "dense-row form of the thread-per-row levels off: the CSR form stays tested"},
    {"IPD_NO_PAD", SW_FLAG, "launch path without the padded rows (bench-workload tests)"},
    {"IPD_NO_STAGE", SW_FLAG, "launch path without LDS staging of the gather vectors (bench-workload tests)"},
    {"IPD_NO_RRC", SW_FLAG, "launch path without the fused residual + restriction (bench-workload tests)"},
    {"IPD_NO_GRAPH", SW_FLAG, "launch path without graph replay (bench-workload tests)"},
    {"IPD_NO_MIS_SMALL", SW_FLAG, "the two forms of mis_set compared bit for bit (tests)"},
    {"IPD_PRODUCT", SW_VALUE, "rows|tiles: the two forms of the ordered product compared bit for bit (tests)"},
    {"IPD_INTERP", SW_VALUE, "single|split|block: the forms of the interpolation build compared bit for bit (tests)"},
    {"IPD_MASKOP", SW_FLAG, "mask sweeps on the launch path below the 4 M-entry policy threshold (tests)"},
    {"IPD_NO_DONOR", SW_FLAG, "AMG4POT's shared levels 1-2 off: the bit-identity tests"},
    {"IPD_NO_STEP_DONOR", SW_FLAG, "the drivers' step donors off: the bit-identity tests"},
    {"IPD_NO_POT_CONCURRENT", SW_FLAG, "AMG4POT's two concurrent solves off: the bit-identity tests"},
    {"IPD_COST_STORE", SW_VALUE, "8|16: the store width of the point-cloud cost build where both are possible (measurement, tests)"},
    {"IPD_APD_REPS", SW_VALUE, "1|2|4|8: column chunks a wave of the drivers' tile walker takes (ipd_apd_geo.h), read when a workspace is created; the natural rule leaves 1 below about 1793 x 16353 entries, so this is how tests run the rep loop and its partly filled last group at small shapes"},
    {"IPD_SHARD_EMULATE", SW_VALUE, "<G>: one process plays G row-block owners (the sharded path's test on one GPU)"},
    {"IPD_DEBUG_SKIP", SW_VALUE, "<mask>: timing by elimination inside the tail's sub-cycle (results void)"},
    {"IPD_PROFILE", SW_VALUE, "phase wall clocks (ipd_prof_read); on unless empty or starting with '0'"},
    {"IPD_DEBUG_LEVELS", SW_FLAG, "the planner's decisions on stderr"},
    {"IPD_DUMP_SYSTEM", SW_VALUE, "<prefix>: writes the Newton systems of the Hybrid_AMG calls below (tests/read_system_dump.py)"},
    {"IPD_DUMP_CALLS", SW_VALUE, "<lo>-<hi>: the calls IPD_DUMP_SYSTEM writes"},
};

static inline bool switch_known(const char* name, SwitchKind kind) {
    for (const SwitchInfo& s : IPD_SWITCHES)
        if (!std::strcmp(s.name, name)) return s.kind == kind;
    return false;
}

// flag switch: set and starting with '1'
static inline bool switch_on(const char* name) {
    assert(switch_known(name, SW_FLAG));
    const char* e = std::getenv(name);
    return e && e[0] == '1';
}

// value switch: its value, nullptr when unset
static inline const char* switch_value(const char* name) {
    assert(switch_known(name, SW_VALUE));
    return std::getenv(name);
}
