// CPU driver of the launch planner (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_launch_plan.h) for
// tests/test_launch_plan.py.  One case per input line:
//   <J> <cu> <switches|-> <donor levels d> then d times <S> <L> <G> <lanes> then J times
//   <nr> <nnz> <nf> <maxoff> <pt_nr> <pt_nc> <pt_nnz> <p_nr> <p_nc> <p_nnz> <t1> <t1_nr> <t1_nnz>
// (switches: comma-separated IPD_NO_PAD, IPD_NO_STAGE, IPD_NO_RRC).  Per case it prints the record of
// every level as launch_plan_line writes it (what IPD_DEBUG_LEVELS shows), then
//   end
// The first line of the output is
//   limits <BT> <STAGE_MAX> <ROW_U> <QUEUED_NNZ_MAX> <RRC_T1_NNZ_MAX>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_launch_plan.h"

int main() {
    std::printf("limits %d %d %d %d %d\n", BT, STAGE_MAX, ROW_U, (int)QUEUED_NNZ_MAX, RRC_T1_NNZ_MAX);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int J = 0, cu = 0, d = 0;
        std::string sws;
        if (!(in >> J >> cu >> sws >> d)) continue;
        LaunchSwitches sw;
        const struct {
            const char* name;
            bool* flag;
        } names[] = {{"IPD_NO_PAD", &sw.no_pad}, {"IPD_NO_STAGE", &sw.no_stage}, {"IPD_NO_RRC", &sw.no_rrc}};
        std::istringstream swin(sws);
        for (std::string s; std::getline(swin, s, ',');) {
            bool known = s == "-";
            for (const auto& n : names)
                if (s == n.name) known = *n.flag = true;
            if (!known) {
                std::fprintf(stderr, "unknown switch %s\n", s.c_str());
                return 2;
            }
        }
        LaunchLevel donor[3];
        for (int k = 1; k <= d && k <= 2; ++k) in >> donor[k].S >> donor[k].L >> donor[k].G >> donor[k].lanes;
        std::vector<LaunchShape> L((size_t)J + 1);
        for (int k = 1; k <= J; ++k) {
            LaunchShape& s = L[(size_t)k];
            int t1 = 0;
            in >> s.nr >> s.nnz >> s.nf >> s.maxoff >> s.Pt.nr >> s.Pt.nc >> s.Pt.nnz >> s.P.nr >> s.P.nc >> s.P.nnz >> t1 >>
                s.T1.nr >> s.T1.nnz;
            s.t1 = t1 != 0;
        }
        if (!in || d > 2) {
            std::fprintf(stderr, "bad case line\n");
            return 2;
        }
        const std::vector<LaunchLevel> plan = plan_launches(L.data(), J, cu, sw, d ? donor : nullptr, d);
        for (int k = 1; k <= J; ++k) std::printf("%s\n", launch_plan_line(plan[(size_t)k], k, J).c_str());
        std::printf("end\n");
    }
    return 0;
}
