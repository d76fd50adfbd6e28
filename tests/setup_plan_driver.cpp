// CPU driver of the setup's planner (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_setup_plan.h) for
// tests/test_setup_plan.py and tests/test_gpu_setup_at_scale.py.  One query per input line:
//   rowcount <lazy> <nr> <producer_has_tail>
//   transfer <switches> <level> <N> <nnz> <Nc> <bigph> <fnode> <inter> <hint0> <hint1> <hint2> <hint3>
//   product  <switches> <lazy> <x_maxrow> <x_nr> <x_nc> <x_nnz> <y_nr> <y_nc> <y_nnz>
// switches: - or a comma-separated list of IPD_INTERP=<value>, IPD_PRODUCT=<value>, IPD_NO_MIS_SMALL, parsed by the
// function the library hands the environment's values to.  Per query it prints one line:
//   rowcount <MODE>
//   transfer_plan_line(...) followed by mis_small=<0|1>, the decision taken before the split
//   product tiles= edge= threads= rows= bound= bytes= modelled= t_rows= t_tiles=
// The first line of the output is
//   limits SPGEMM_LAZY_MAX= SCAN_HEAD_MAX= MIS_SMALL_ROWS= MIS_SMALL_NNZ= SPLIT_ROW_MIN= WIDE_ROW_MIN= XFER_HINT_LEVELS= SPGEMM_TILE=
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_setup_plan.h"

static bool parse_switches(const std::string& list, SetupSwitches* sw) {
    std::string interp, product;
    bool has_interp = false, has_product = false, no_mis_small = false;
    std::istringstream in(list);
    for (std::string s; std::getline(in, s, ',');) {
        if (s == "-") continue;
        if (s.rfind("IPD_INTERP=", 0) == 0)
            interp = s.substr(11), has_interp = true;
        else if (s.rfind("IPD_PRODUCT=", 0) == 0)
            product = s.substr(12), has_product = true;
        else if (s == "IPD_NO_MIS_SMALL")
            no_mis_small = true;
        else
            return false;
    }
    *sw = setup_switches(has_interp ? interp.c_str() : nullptr, has_product ? product.c_str() : nullptr, no_mis_small);
    return true;
}

int main() {
    std::printf("limits SPGEMM_LAZY_MAX=%zu SCAN_HEAD_MAX=%d MIS_SMALL_ROWS=%d MIS_SMALL_NNZ=%d SPLIT_ROW_MIN=%g "
                "WIDE_ROW_MIN=%g XFER_HINT_LEVELS=%d SPGEMM_TILE=%d\n",
                SPGEMM_LAZY_MAX, SCAN_HEAD_MAX, MIS_SMALL_ROWS, MIS_SMALL_NNZ, SPLIT_ROW_MIN, WIDE_ROW_MIN,
                XFER_HINT_LEVELS, SPGEMM_TILE);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what, sws;
        if (!(in >> what)) continue;
        SetupSwitches sw;
        if (what == "rowcount") {
            int lazy = 0, nr = 0, tail = 0;
            in >> lazy >> nr >> tail;
            if (in) std::printf("rowcount %s\n", ROW_COUNT_NAMES[plan_row_count(lazy != 0, nr, tail != 0)]);
        } else if (what == "transfer") {
            TransferShape s;
            int Nc = 0;
            in >> sws >> s.level >> s.N >> s.nnz >> Nc >> s.bigph >> s.fnode >> s.inter >> s.hint[0] >> s.hint[1] >>
                s.hint[2] >> s.hint[3];
            if (in && parse_switches(sws, &sw))
                std::printf("%s mis_small=%d\n", transfer_plan_line(s, Nc, plan_transfer(s, Nc, sw)).c_str(),
                            (int)plan_mis_small(s.N, s.nnz, sw));
            else
                in.setstate(std::ios::failbit);
        } else if (what == "product") {
            ProductShape X, Y;
            int lazy = 0, x_maxrow = 0;
            in >> sws >> lazy >> x_maxrow >> X.nr >> X.nc >> X.nnz >> Y.nr >> Y.nc >> Y.nnz;
            if (in && parse_switches(sws, &sw)) {
                const ProductPlan p = plan_product(X, Y, x_maxrow, sw.product, lazy != 0);
                std::printf("product tiles=%d edge=%d threads=%d rows=%s bound=%zu bytes=%zu modelled=%d t_rows=%.3f "
                            "t_tiles=%.3f\n", (int)p.tiles, p.edge, p.threads, ROW_COUNT_NAMES[p.rows], p.bound, p.bytes,
                            (int)p.modelled, p.t_rows, p.t_tiles);
            } else
                in.setstate(std::ios::failbit);
        } else
            in.setstate(std::ios::failbit);
        if (!in) {
            std::fprintf(stderr, "bad query: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
