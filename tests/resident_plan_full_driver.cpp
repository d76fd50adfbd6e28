// CPU driver of resident_takes_full (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_resident_plan.h) for
// tests/test_resident_plan_full.py.  One case per input line:
//   <nf> <nc> <N2> <Nt> <cycle> <smoth> <G override, 0 = none> <poly2> <mask transfers> <wident> <isnsp> <localfirst> <no_full>
// A three-level hierarchy with dense rows (the padded copies as wide as the longest row) is planned as the library
// plans it -- plan_resident, then resident_takes_poly2 where the composed level 2 is asked for -- and per case it
// prints what the plan dump of tests/resident_plan_driver.cpp shows of the key, with the new field behind it:
//   plan <kind> <ke> <ke3> <poly2> <G> <wident> full <0|1>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_resident_plan.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int nf, nc, N2, Nt, smoth, G, poly2, xm, wident, isnsp, lfirst, no_full;
        std::string cycle;
        if (!(in >> nf >> nc >> N2 >> Nt >> cycle >> smoth >> G >> poly2 >> xm >> wident >> isnsp >> lfirst >> no_full)) continue;
        LevelShape L[4];
        L[1].nr = nf + nc;
        L[1].nf = nf;
        L[1].maxoff = std::max(nf, nc);
        L[1].nnz = 2 * nf * nc + nf + nc;
        L[2].nr = N2;
        L[2].maxoff = N2 - 1;
        L[2].nnz = N2 * N2;
        L[2].p_nnz = nf * nc + nc;
        L[3].nr = Nt;
        L[3].nnz = Nt * Nt;
        L[3].p_nnz = N2;
        ResidentInputs ri;
        ri.L = L;
        ri.J = 3;
        ri.S[1] = pad_stride(L[1].maxoff);
        ri.S[2] = pad_stride(L[2].maxoff);
        ri.cycle = cycle[0];
        ri.smoth = smoth;
        ri.bigph = true;
        ri.num_cu = 256;
        PlanSwitches sw;
        sw.resident_g = G;
        sw.res_no_full = no_full != 0;
        ResidentPlan p = plan_resident(ri, sw);
        if (poly2 && resident_takes_poly2(p, ri)) p.key.poly2 = true;
        const ResidentFullFacts facts{xm != 0, wident, isnsp, lfirst != 0};
        static const char* const kinds[] = {"none", "k", "big", "deep"};
        std::printf("plan %s %d %d %d %d %d full %d\n", kinds[p.kind], p.key.ke, p.key.ke3, (int)p.key.poly2, p.G, p.wident,
                    (int)resident_takes_full(p, ri, facts, sw));
    }
    return 0;
}
