// CPU driver of the level planner (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_level_plan.h) for
// tests/test_level_plan.py.  One case per input line:
//   <J> <cycle> <smoth> <twogrid> <concurrent_pair> <switches|-> then J times <nr> <nnz> <nf> <maxoff> <p_nnz>
// (switches: comma-separated IPD_NO_* names).  Per case it prints
//   plan <small_ok> <k_sub> <sub_semi_root> <sub5 role> <use_poly> <tiny_lo>
//   image <role> <k_lds> <k_semi> <k_tiny> <k_blk> <stage> <lds> <rows of its largest thread-per-row level k >= 2>
//   end
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_level_plan.h"

// SOL_HEAD of the gfx950 build: sol_r16(sizeof(SolveDesc)) + sol_r16(4 * RELOC_MAX)
static constexpr size_t SOL_HEAD_GFX950 = 12592;

int main() {
    static const char* const roles[] = {"solve", "sub", "sub3", "sub4", "none"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int J = 0, smoth = 0, twogrid = 0, pair = 0;
        std::string cycle, sws;
        if (!(in >> J >> cycle >> smoth >> twogrid >> pair >> sws)) continue;
        PlanOptions o;
        o.cycle = cycle[0];
        o.smoth = smoth;
        o.twogrid = twogrid != 0;
        o.concurrent_pair = pair != 0;
        o.sol_head = SOL_HEAD_GFX950;
        PlanSwitches sw;
        const struct {
            const char* name;
            bool* flag;
        } names[] = {{"IPD_NO_POLY", &sw.no_poly},
                     {"IPD_NO_BLK", &sw.no_blk},
                     {"IPD_NO_BPOLY", &sw.no_bpoly},
                     {"IPD_NO_BLKDENSE", &sw.no_blkdense},
                     {"IPD_NO_SMALL", &sw.no_small},
                     {"IPD_NO_SUBCYCLE", &sw.no_subcycle},
                     {"IPD_NO_RESIDENT", &sw.no_resident},
                     {"IPD_NO_RESIDENT_REMOTE", &sw.no_resident_remote},
                     {"IPD_NO_RESIDENT_THREE", &sw.no_resident_three},
                     {"IPD_NO_RESIDENT_DEEP", &sw.no_resident_deep},
                     {"IPD_NO_RESIDENT_BIG", &sw.no_resident_big},
                     {"IPD_NO_RES_POLY4", &sw.no_res_poly4}};
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
        std::vector<LevelShape> L((size_t)J + 1);
        for (int k = 1; k <= J; ++k) in >> L[k].nr >> L[k].nnz >> L[k].nf >> L[k].maxoff >> L[k].p_nnz;
        if (!in) {
            std::fprintf(stderr, "short case line\n");
            return 2;
        }
        const LevelPlan p = plan_levels(L.data(), J, o, sw);
        std::printf("plan %d %d %d %s %d %d\n", (int)p.small_ok, p.k_sub, (int)p.sub_semi_root, roles[p.sub5],
                    (int)p.use_poly, p.tiny_lo);
        for (const ImageSpec& s : p.images) {
            int tpr = 0;
            for (int k = 2; k <= J; ++k)
                if (p.thread_per_row(s, k)) tpr = std::max(tpr, L[k].nr);
            std::printf("image %s %d %d %d %d %zu %zu %d\n", roles[s.role], s.k_lds, s.k_semi, s.k_tiny, s.k_blk,
                        s.stage_bytes, s.lds, tpr);
        }
        std::printf("end\n");
    }
    return 0;
}
