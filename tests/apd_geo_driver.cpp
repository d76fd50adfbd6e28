// CPU driver of the tile walker's host-clean geometry header (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_apd_geo.h)
// for tests/test_apd_geo.py.  One query per input line:
//   geo <m> <n> <IPD_APD_REPS value or ->      the plan of a workspace and its buffer sizes
//   cover <m> <n> <IPD_APD_REPS value or ->    walks the columns as k_tiles does
//   switch <value or ->
// Per query it prints one line:
//   geo nib= njg= reps= nblk= lpart= rpart=
//   cover min=<fewest (jg, rep, column-in-chunk) owners of a column j < n> max=<most> broke=<walks ended by j0 >= n>
//         idle=<chunks not walked after such an end> nib= njg= reps=
//   switch <0: natural | 1|2|4|8 | -1: refused>
// The first line of the output is
//   limits TR= TC= APD_WAVES= APD_REPS_MAX=
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_apd_geo.h"

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d APD_REPS_MAX=%d\n", TR, TC, APD_WAVES, APD_REPS_MAX);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "switch") {
            std::string sw;
            if (!(in >> sw)) continue;
            std::printf("switch %d\n", apd_reps_switch(sw == "-" ? nullptr : sw.c_str()));
            continue;
        }
        int m = 0, n = 0;
        std::string sw;
        in >> m >> n >> sw;
        if (!in || m < 1 || n < 1) continue;
        const int forced = apd_reps_switch(sw == "-" ? nullptr : sw.c_str());
        if (forced < 0) {
            std::printf("%s refused\n", what.c_str());
            continue;
        }
        const Geo g = make_geo(m, n, forced);
        if (what == "geo") {
            std::printf("geo nib=%d njg=%d reps=%d nblk=%zu lpart=%zu rpart=%zu\n", g.nib, g.njg, g.reps, apd_nblk(g),
                        apd_lpart_len(g), apd_rpart_len(g));
        } else if (what == "cover") {
            // the columns do not depend on the row block: one wave's walk per column group
            std::vector<int> owners((size_t)n, 0);
            long long broke = 0, idle = 0;
            for (int jg = 0; jg < g.njg; ++jg)
                for (int rep = 0; rep < g.reps; ++rep) {
                    const int j0 = apd_step_col(g, jg, rep);
                    if (j0 >= n) {   // k_tiles: if (j0 >= g.n) break;
                        ++broke;
                        idle += g.reps - rep;
                        break;
                    }
                    for (int cc = 0; cc < TC; ++cc) {
                        const int j = j0 + cc;
                        if (j < n) ++owners[(size_t)j];   // k_tiles: if (in_i && j < g.n)
                    }
                }
            int lo = 1 << 30, hi = 0;
            for (int v : owners) {
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            std::printf("cover min=%d max=%d broke=%lld idle=%lld nib=%d njg=%d reps=%d\n", lo, hi, broke, idle, g.nib, g.njg, g.reps);
        }
    }
    return 0;
}
