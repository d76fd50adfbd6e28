// CPU driver of the host rules of the KKT operators (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_kkt_plan.h) for
// tests/test_kkt_plan.py.  The first line of the output is
//   limits <AX_TR> <AX_TC> <AX_LD> <ATY_TC> <ASAT_TILE> <PHI_PARTS_MAX> <ASAT_SMALL_WORDS> <ASAT_SMALL_WGS>
//          <ASAT_SMALL_HINT_MAX> <ASAT_GAVE_UP>
// then one answer line per input line:
//   checkmn <m> <n>            -> <code> <message, or ->       kkt_check_mn (every C ABI entry)
//   asatcheck <m> <n>          -> <code> <message, or ->       asat_check_mn
//   geo <m> <n>                -> <nib> <njb> <M> <ntiles> <col_words> <row_words> <rp_len> <tiles_grid> <rows_grid>
//                                 <diag_grid> <small_lds>
//   wide <m> <address>         -> <0|1>
//   cap <hint> <m> <n>         -> <cap>
//   small <hint> <m> <n>       -> <0|1>
//   accepts <nnz> <cap>        -> <0|1>
//   hint_small <hint> <nnz>    -> <hint>
//   hint_general <nnz>         -> <hint>
//   ax <m> <n>                 -> <nib> <njb> <lpart> <rpart> <final_grid>
//   aty <m> <n> <address>      -> <vec2> <gx> <gy>
//   phi <m> <n>                -> <npart>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_kkt_plan.h"

static void print_check(const KktDimCheck& c) { std::printf("%d %s\n", c.code, c.msg ? c.msg : "-"); }

int main() {
    std::printf("limits %d %d %d %d %d %d %d %d %d %d\n", AX_TR, AX_TC, AX_LD, ATY_TC, ASAT_TILE, PHI_PARTS_MAX,
                ASAT_SMALL_WORDS, ASAT_SMALL_WGS, ASAT_SMALL_HINT_MAX, ASAT_GAVE_UP);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        long long a = 0, b = 0, c = 0;
        in >> a >> b >> c;   // (missing ones stay 0)
        if (cmd == "checkmn") {
            print_check(kkt_check_mn(a, b));
        } else if (cmd == "asatcheck") {
            print_check(asat_check_mn((int)a, (int)b));
        } else if (cmd == "geo") {
            const AsatGeo g = asat_geo((int)a, (int)b);
            std::printf("%d %d %d %d %zu %zu %zu %d %d %d %zu\n", g.nib, g.njb, g.M, g.ntiles, g.col_words(),
                        g.row_words(), g.rp_len(), g.tiles_grid(), g.rows_grid(), g.diag_grid(), g.small_lds());
        } else if (cmd == "wide") {
            std::printf("%d\n", asat_wide((int)a, (uintptr_t)b) ? 1 : 0);
        } else if (cmd == "cap") {
            std::printf("%lld\n", asat_cap(a, (int)b, (int)c));
        } else if (cmd == "small") {
            std::printf("%d\n", asat_small_route(a, asat_geo((int)b, (int)c)) ? 1 : 0);
        } else if (cmd == "accepts") {
            std::printf("%d\n", asat_accepts(a, b) ? 1 : 0);
        } else if (cmd == "hint_small") {
            std::printf("%lld\n", asat_hint_after_small(a, (int)b));
        } else if (cmd == "hint_general") {
            std::printf("%lld\n", asat_hint_after_general((int)a));
        } else if (cmd == "ax") {
            const AxGeo g = ax_geo((int)a, (int)b);
            std::printf("%d %d %zu %zu %d\n", g.nib, g.njb, g.lpart, g.rpart, g.final_grid);
        } else if (cmd == "aty") {
            const bool vec2 = aty_vec2((int)a, (uintptr_t)c);
            std::printf("%d %d %d\n", vec2 ? 1 : 0, aty_grid_x((int)a, vec2), aty_grid_y((int)b));
        } else if (cmd == "phi") {
            std::printf("%d\n", phi_parts((int)a, (int)b));
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
