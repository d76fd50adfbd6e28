// CPU driver of the resident planner (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_resident_plan.h) for
// tests/test_resident_plan.py.  One case per input line:
//   <J> <cycle> <smoth> <twogrid> <bigph> <switches|-> <CUs> <images: plan|none> <S1> <S2> <S3>
//   then J times <nr> <nnz> <nf> <maxoff> <p_nnz>
// (switches: comma-separated IPD_* names, NAME=<n> for the value switches; S: stride of the launches' padded
// copy of levels 1..3, 0 = none; images: the LDS images the level planner packs for these shapes, or none).
// The planners run in the order the library runs them -- plan_resident at set-up, then, as at a mask attach
// with m = the C block and n = the F block, plan_resident_big and plan_resident_deep -- and per case it prints
//   images <role>...                           the images the resident planner was offered
//   resident <prepare|big|deep> <kind> <big> <ke> <ke3> <poly2> <ke2> <rpw> <deep> <G> <grid> <lds> <remote>
//            <three> <poly3> <poly4> <tail_root> <tail_image> <tail_bm> <S1> <S2> <S3> <priv1> <priv2> <priv3>
//            <wident> <ranks> <levels>
//   end
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_resident_plan.h"

static const char* const ROLES[] = {"solve", "sub", "sub3", "sub4", "none"};

static void print_plan(const char* stage, const ResidentPlan& p) {
    static const char* const kinds[] = {"none", "k", "big", "deep"};
    std::printf("resident %s %s %d %d %d %d %d %d %d %d %d %zu %d %d %d %d %d %s %d %d %d %d %d %d %d %d %d %d\n", stage,
                kinds[p.kind], (int)p.key.big, p.key.ke, p.key.ke3, (int)p.key.poly2, p.key.ke2, p.key.rpw,
                (int)p.key.deep, p.G, p.grid(), p.lds, (int)p.remote, (int)p.three, (int)p.poly3, (int)p.poly4,
                p.tail_root, ROLES[p.tail_image], (int)p.tail_bm, p.S[1], p.S[2], p.S[3], (int)p.priv[1], (int)p.priv[2],
                (int)p.priv[3], p.wident, p.ranks, p.levels);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int J = 0, smoth = 0, twogrid = 0, bigph = 0, cus = 0;
        std::string cycle, sws, images;
        ResidentInputs ri;
        if (!(in >> J >> cycle >> smoth >> twogrid >> bigph >> sws >> cus >> images >> ri.S[1] >> ri.S[2] >> ri.S[3])) continue;
        PlanSwitches sw;
        const struct {
            const char* name;
            bool* flag;
            int* value;
        } names[] = {{"IPD_NO_POLY", &sw.no_poly, nullptr},
                     {"IPD_NO_BLK", &sw.no_blk, nullptr},
                     {"IPD_NO_BPOLY", &sw.no_bpoly, nullptr},
                     {"IPD_NO_BLKDENSE", &sw.no_blkdense, nullptr},
                     {"IPD_NO_SMALL", &sw.no_small, nullptr},
                     {"IPD_NO_SUBCYCLE", &sw.no_subcycle, nullptr},
                     {"IPD_NO_RESIDENT", &sw.no_resident, nullptr},
                     {"IPD_NO_RESIDENT_REMOTE", &sw.no_resident_remote, nullptr},
                     {"IPD_NO_RESIDENT_THREE", &sw.no_resident_three, nullptr},
                     {"IPD_NO_RESIDENT_DEEP", &sw.no_resident_deep, nullptr},
                     {"IPD_NO_RESIDENT_BIG", &sw.no_resident_big, nullptr},
                     {"IPD_NO_RES_POLY4", &sw.no_res_poly4, nullptr},
                     {"IPD_RESIDENT_BIG", &sw.resident_big, nullptr},
                     {"IPD_RESIDENT_G", nullptr, &sw.resident_g},
                     {"IPD_RESIDENT_RANKS", nullptr, &sw.resident_ranks}};
        std::istringstream swin(sws);
        for (std::string s; std::getline(swin, s, ',');) {
            bool known = s == "-";
            const size_t eq = s.find('=');
            for (const auto& n : names) {
                if (n.flag && s == n.name) known = *n.flag = true;
                if (n.value && eq != std::string::npos && s.substr(0, eq) == n.name) {
                    *n.value = std::atoi(s.c_str() + eq + 1);
                    known = true;
                }
            }
            if (!known) {
                std::fprintf(stderr, "unknown switch %s\n", s.c_str());
                return 2;
            }
        }
        std::vector<LevelShape> L((size_t)J + 1);
        for (int k = 1; k <= J; ++k) in >> L[k].nr >> L[k].nnz >> L[k].nf >> L[k].maxoff >> L[k].p_nnz;
        if (!in || (images != "plan" && images != "none")) {
            std::fprintf(stderr, "bad case line\n");
            return 2;
        }
        ri.L = L.data();
        ri.J = J;
        ri.cycle = cycle[0];
        ri.smoth = smoth;
        ri.twogrid = twogrid != 0;
        ri.bigph = bigph != 0;
        ri.num_cu = cus;
        std::printf("images");
        if (images == "plan") {
            PlanOptions o;
            o.cycle = ri.cycle;
            o.smoth = smoth;
            o.twogrid = ri.twogrid;
            const LevelPlan lp = plan_levels(L.data(), J, o, sw);
            ri.small_ok = lp.small_ok;
            ri.k_sub = lp.k_sub;
            ri.sub5 = lp.sub5;
            for (const ImageSpec& s : lp.images) {
                if (s.role == IMG_SOLVE) continue;
                ri.img[s.role].have = true;
                ri.img[s.role].lds = s.lds;
                std::printf(" %s", ROLES[s.role]);
            }
        }
        std::printf("\n");
        const ResidentPlan p0 = plan_resident(ri, sw);
        print_plan("prepare", p0);
        // (a transfer to be checked on the device is taken to pass)
        ResidentFacts f{J >= 1 ? L[1].nr - L[1].nf : 0, J >= 1 ? L[1].nf : 0, sw.no_resident, p0.kind != RESIDENT_NONE, false,
                        p0.wident != 0};
        const ResidentPlan pb = plan_resident_big(ri, sw, f);
        print_plan("big", pb);
        f.mask_form = pb.kind != RESIDENT_NONE;
        print_plan("deep", plan_resident_deep(ri, sw, f));
        std::printf("end\n");
    }
    return 0;
}
