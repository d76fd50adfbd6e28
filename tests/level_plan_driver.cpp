// CPU driver of the level planner (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_level_plan.h) for
// tests/test_level_plan.py.  One case per input line:
//   <J> <cycle> <smoth> <twogrid> <concurrent_pair> <switches|-> then J times <nr> <nnz> <nf> <maxoff> <p_nnz>
// (switches: comma-separated IPD_NO_* names).  Per case it prints
//   plan <small_ok> <k_sub> <sub_semi_root> <sub5 role> <use_poly> <tiny_lo>
//   image <role> <k_lds> <k_semi> <k_tiny> <k_blk> <stage> <lds> <rows of its largest thread-per-row level k >= 2>
//   end
// and, between an image line and the next, the image as image_layout lays it out (none for a solve with
// nothing cached):
//   level <k> <form> <rows>                       one per level of the image
//   piece <level> <slot> <kind> <bytes> <offset>  in the order of the image
//   layout <image_bytes> <total> <relocations> <k_cached> then the named reserves of the prediction:
//          <head> <xx> <bp_part> <child_pad> <coarsest_lmap> <const_pad> <above_root>
// The first line of the output is
//   limits <IMAGE_LDS_BUDGET> <IMAGE_LDS_OPTIN> <RELOC_MAX> <SOL_HEAD> <BT>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_level_plan.h"

static const char* const SLOT_NAMES[SLOT_COUNT] = {
    "rp", "ci", "va", "dinv", "Axi", "xx", "rest.rp", "rest.ci", "rest.va", "prol.rp", "prol.ci", "prol.va",
    "lmap", "dA", "dP", "dPt", "pMr", "pMe", "pMc", "pW", "r", "e", "e2", "rr", "w",
    "bp_part", "pcg.work", "rest.x", "rest.y", "pcg.rp", "pcg.ci", "pcg.va"};
static const char* const KIND_NAMES[] = {"copy", "dense", "lmap", "poly", "work", "alias"};

// What the prediction s.lds holds beyond the layout's total, term by term, from the header's names: the reserves
// plan_lds counted for the levels it cached (level_reserves), less what the layout does carve of them
static ImageReserves image_reserves(const LevelShape* L, const LevelPlan& plan, const ImageSpec& s, const ImageLayout& lay) {
    ImageReserves r;
    r.of[RSV_HEAD] = RESERVE_HEAD;
    for (int k = s.k_cached; k <= plan.J; ++k) {
        const ImageSpec a = level_alone(k, plan.tiny_lo);
        const bool below = k >= 2 && block_wide(plan.form(level_alone(k - 1, plan.tiny_lo), k - 1));
        const LevelPieces counted = level_pieces(L, plan.J, a, plan.lean_vectors, k, plan.form(a, k), false);
        const ImageReserves lr = level_reserves(counted, below);
        for (int q = 0; q < RSV_COUNT; ++q) r.of[q] += lr.of[q];
        if (k < s.k_lds)
            r.of[RSV_ABOVE_ROOT] += counted.sum();
        else
            r.of[RSV_CHILD_PAD] -= plan.pieces(L, s, k).sum() - counted.sum();   // the padding that is carved
    }
    if (const ImagePiece* bp = lay.find(0, SLOT_BP_PART)) r.of[RSV_BP_PART] -= plan_r16(bp->bytes);
    return r;
}

int main() {
    static const char* const roles[] = {"solve", "sub", "sub3", "sub4", "none"};
    static const char* const forms[] = {"semi", "csr", "bdense", "tiny", "poly", "lpoly", "bpoly"};
    std::printf("limits %zu %zu %d %zu %d\n", IMAGE_LDS_BUDGET, IMAGE_LDS_OPTIN, RELOC_MAX, SOL_HEAD, BT);
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
            if (s.k_lds > J) continue;
            const ImageLayout lay = image_layout(L.data(), p, s);
            for (int k = s.k_lds; k <= J; ++k) std::printf("level %d %s %d\n", k, forms[p.form(s, k)], L[k].nr);
            for (const ImagePiece& q : lay.pieces)
                std::printf("piece %d %s %s %zu %zu\n", q.level, SLOT_NAMES[q.slot], KIND_NAMES[q.kind], q.bytes,
                            q.off);
            const ImageReserves r = image_reserves(L.data(), p, s, lay);
            std::printf("layout %zu %zu %zu %d", lay.image_bytes, lay.total, lay.pieces.size(), s.k_cached);
            for (size_t v : r.of) std::printf(" %zu", v);
            std::printf("\n");
        }
        std::printf("end\n");
    }
    return 0;
}
