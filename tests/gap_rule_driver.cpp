// CPU driver of the gap rule's decisions in the drivers' host-clean script header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_apd_script.h) for tests/test_gap_rule.py.  One query per input line, one
// line of output per query; a double goes in and out as a C hexadecimal literal (%a), so the test compares bits.
//   due <k> <first> <every> <converged>          -> due 0|1
//   lower <dual0> <dual1>                        -> lower side
//   upper <ok0> <fval0> <ok1> <fval1>            -> upper side
//   best <lower> <best>                          -> best improves value
//   thr <gap_tol> <gap_rel> <upper>              -> thr value
//   gap <upper> <best>                           -> gap value
//   stop <thr> <upper_ok> <gap>                  -> stop 0|1
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_apd_script.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, tok;
        if (!(in >> what)) continue;
        std::vector<double> a;
        while (in >> tok) a.push_back(std::strtod(tok.c_str(), nullptr));
        auto need = [&](size_t n) {
            if (a.size() >= n) return true;
            std::printf("%s short\n", what.c_str());
            return false;
        };
        if (what == "due") {
            if (!need(4)) continue;
            std::printf("due %d\n", apd_gap_due((int)a[0], (int)a[1], (int)a[2], a[3] != 0.0) ? 1 : 0);
        } else if (what == "lower") {
            if (!need(2)) continue;
            std::printf("lower %d\n", apd_gap_lower_side(a[0], a[1]));
        } else if (what == "upper") {
            if (!need(4)) continue;
            std::printf("upper %d\n", apd_gap_upper_side((int)a[0], a[1], (int)a[2], a[3]));
        } else if (what == "best") {
            if (!need(2)) continue;
            std::printf("best %d %a\n", apd_gap_improves(a[0], a[1]) ? 1 : 0, apd_gap_best(a[0], a[1]));
        } else if (what == "thr") {
            if (!need(3)) continue;
            std::printf("thr %a\n", apd_gap_threshold(a[0], a[1], a[2]));
        } else if (what == "gap") {
            if (!need(2)) continue;
            std::printf("gap %a\n", apd_gap_value(a[0], a[1]));
        } else if (what == "stop") {
            if (!need(3)) continue;
            std::printf("stop %d\n", apd_gap_stops(a[0], (int)a[1], a[2]) ? 1 : 0);
        } else {
            std::printf("%s unknown\n", what.c_str());
        }
    }
    return 0;
}
