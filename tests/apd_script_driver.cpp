// CPU driver of the drivers' host-clean script header (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_apd_script.h) for
// tests/test_apd_script.py.  One query per input line, one line of output per query; a double goes in and out as a C
// hexadecimal literal (%a), so the test compares bits.
//   step <k> <bk> <cls> <tol1>              -> step ak bk1 tk ssn_tol stall
//   warm <gk> <bk> <muf> <iters>            -> warm, then per iteration the 12 WarmScal fields, sg, gk1, bk1
//   merit <merit3> <bk1> <tk> <lam2> <wlk_lam> <prox2> <z2> <zmp2>   -> merit value
//   accept <cls> <bk1> <resk> <kk x4> <kkt0 x4>   -> accept max_rr resk_of_kk restarts bk_next_class2
//   stop <cls> <normF_old> <normF_new> <ssn_tol> <ssn_it> <ssn_it_max>   -> stop wants_step solved stalled exhausted
//   route <cls> <inner_solver>              -> route NAME
//   evalkind <cls> <gama vector> <merit3>   -> evalkind NAME
//   bytes <m> <n> <phi> <gama>              -> bytes value
//   ls <arm> <delta> <nu> <ress> <cF_old> <ll_max> <merit3> <tail> <cF(0)> <cF(1)> ...
//        the line search of one Newton step over the merit sequence cF(ll) (`tail` from the end of the list on).
//        arm = auto: as apd_iterate -- the first trial, then the arm apd_ls_batched selects;
//        arm = batched | sequential: that arm after a rejected first trial, whatever the rule says.
//        -> ls arm=<none|batched|sequential> ll= step= passes=<merit passes or further evaluations>
// The first line of the output is
//   limits MK=
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_apd_script.h"

static const char* const ROUTE_NAMES[] = {"DIRECT",  "DIRECT_POT", "PCG",        "PCG_POT",
                                          "AUG_PCG", "PCG4POT",    "HYBRID_AMG", "AMG4POT"};
static const char* const EVAL_NAMES[] = {"CLS2", "GVEC_M3", "GVEC", "GS_M3", "GS"};

int main() {
    std::printf("limits MK=%d\n", MK);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, tok;
        if (!(in >> what)) continue;
        std::vector<std::string> words;
        std::vector<double> a;
        while (in >> tok) {
            words.push_back(tok);
            a.push_back(std::strtod(tok.c_str(), nullptr));
        }
        auto need = [&](size_t n) {
            if (a.size() >= n) return true;
            std::printf("%s short\n", what.c_str());
            return false;
        };
        if (what == "step") {
            if (!need(4)) continue;
            const int k = (int)a[0];
            const bool cls2 = (int)a[2] == 2;
            const ApdStep s = apd_step(k, a[1]);
            const double tol = apd_ssn_tol(k, s.bk1, a[3]);
            std::printf("step %a %a %a %a %a\n", s.ak, s.bk1, s.tk, tol, apd_stall_bound(cls2, tol));
        } else if (what == "warm") {
            if (!need(4)) continue;
            double gk = a[0], bk = a[1];
            std::printf("warm");
            for (int it = 0; it < (int)a[3]; ++it) {
                const WarmStep w = apd_warm_step(gk, bk, a[2]);
                const WarmScal& s = w.s;
                std::printf(" %a %a %a %a %a %a %a %a %a %a %a %a %a %a %a", s.ak, s.gk, s.muf, s.etafk, s.sgk, s.ibk,
                            s.akbk, s.ak2, s.tt_etafk, s.prox_scale, s.gkmu, s.iak1, w.sg, w.gk1, w.bk1);
                gk = w.gk1;
                bk = w.bk1;
            }
            std::printf("\n");
        } else if (what == "merit") {
            if (!need(8)) continue;
            std::printf("merit %a\n", apd_merit_value(a[0] != 0.0, a[1], a[2], a[3], a[4], a[5], a[6], a[7]));
        } else if (what == "accept") {
            if (!need(11)) continue;
            const bool cls2 = (int)a[0] == 2;
            const double rr = apd_max_rr(cls2, &a[3], &a[7]);
            std::printf("accept %a %a %d %a\n", rr, apd_resk(cls2, &a[3]), apd_restarts(a[1], rr, a[2]) ? 1 : 0,
                        apd_restart_bk_class2(a[1]));
        } else if (what == "stop") {
            if (!need(6)) continue;
            const bool cls2 = (int)a[0] == 2;
            std::printf("stop %d %d %d %d\n", apd_ssn_wants_step(a[2], a[3]) ? 1 : 0, apd_ssn_solved(a[2], a[3]) ? 1 : 0,
                        apd_ssn_stalled(cls2, a[1], a[2], a[3]) ? 1 : 0, apd_ssn_exhausted((int)a[4], (int)a[5]) ? 1 : 0);
        } else if (what == "route") {
            if (!need(2)) continue;
            std::printf("route %s\n", ROUTE_NAMES[apd_route((int)a[0] == 2, (int)a[1])]);
        } else if (what == "evalkind") {
            if (!need(3)) continue;
            std::printf("evalkind %s\n", EVAL_NAMES[apd_eval_kind((int)a[0] == 2, a[1] != 0.0, a[2] != 0.0)]);
        } else if (what == "bytes") {
            if (!need(4)) continue;
            std::printf("bytes %a\n", apd_eval_bytes(make_geo((int)a[0], (int)a[1]), a[2] != 0.0, a[3] != 0.0));
        } else if (what == "ls") {
            if (!need(9)) continue;
            const std::string arm = words[0];
            const double delta = a[1], nu = a[2], ress = a[3], cF_old = a[4], tail = a[7];
            const int ll_max = (int)a[5];
            const bool merit3 = a[6] != 0.0;
            auto cF = [&](int ll) { return (size_t)(8 + ll) < a.size() ? a[(size_t)(8 + ll)] : tail; };
            // apd_iterate from "// :182-211 line search" on, with cF(ll) in place of merit(apd_eval(.. step ..))
            int ll = 0, passes = 0;
            double step = 1.0;
            double cF_new = cF(0);
            const bool rejected = apd_armijo_rejects(cF_new, cF_old, nu, step, ress);
            const bool batched = arm == "auto" ? apd_ls_batched(rejected, merit3, ll_max) : rejected && arm == "batched";
            const char* took = "none";
            if (batched) {
                took = "batched";
                bool found = false;
                while (!found && ll < ll_max) {
                    double st[MK], mv[MK];
                    apd_batch_steps(delta, ll, st);
                    for (int k = 0; k < MK; ++k) mv[k] = cF(ll + 1 + k);   // apd_merit
                    ++passes;
                    found = apd_batch_pick(mv, st, cF_old, nu, ress, ll_max, &ll);
                }
                ll = apd_ls_clamp(ll, ll_max);
                step = apd_trial_step(delta, ll);
            } else {
                while (apd_armijo_rejects(cF_new, cF_old, nu, step, ress)) {
                    took = "sequential";
                    ++ll;
                    step = apd_trial_step(delta, ll);
                    cF_new = cF(ll);
                    ++passes;
                    if (ll == ll_max) break;
                    if (ll > 100000) break;   // (a test that asks for ll_max = 0 here would never end)
                }
            }
            std::printf("ls arm=%s ll=%d step=%a passes=%d\n", took, ll, step, passes);
        } else {
            std::printf("%s unknown\n", what.c_str());
        }
    }
    return 0;
}
