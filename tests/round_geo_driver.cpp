// CPU driver of the primal certificate's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_round_geo.h) for tests/test_round_geo.py.  One query per input line,
// `<what> <m> <n>`:
//   geo     the grid, the buffer sizes and the scratch of a call
//   reach   walks every index of the scalars the walking kernel writes and the last kernel reads
// (the walk of the rows and the columns and the row and column partials: tests/walk_geo_driver.cpp)
// Per query it prints one line:
//   geo nib= ng= nslot= rows= cols= blocks= scal= scratch=
//   reach sw=<largest scalar partial written> sr=<largest read> sunwritten= sdup= slen= outside=
// The first line of the output is
//   limits TR= TC= APD_WAVES= WK_CPG= RD_NS= RD_NVEC= RD_SCAL_PASSES= RD_RESULT_DOUBLES=
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "geo_buf.h"
#include "ipd_round_geo.h"

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d WK_CPG=%d RD_NS=%d RD_NVEC=%d RD_SCAL_PASSES=%d RD_RESULT_DOUBLES=%d\n",
                TR, TC, APD_WAVES, WK_CPG, RD_NS, RD_NVEC, RD_SCAL_PASSES, RD_RESULT_DOUBLES);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int m = 0, n = 0;
        if (!(in >> what >> m >> n) || m < 1 || n < 1) continue;
        const RdGeo g = walk_make_geo(m, n);
        if (what == "geo") {
            std::printf("geo nib=%d ng=%d nslot=%d rows=%zu cols=%zu blocks=%d scal=%zu scratch=%zu\n", g.nib, g.ng,
                        g.nslot, walk_row_part_len(g), walk_col_part_len(g), walk_blocks(g), rd_scal_len(g), round_scratch_bytes(g));
        } else if (what == "reach") {
            Buf scal(rd_scal_len(g));
            // k_rd_walk: workgroup (ib, grp) stores its RD_NS sums; k_rd_last reads workgroup k's at k*RD_NS + 0 ..
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ib = 0; ib < g.nib; ++ib)
                    for (int k = 0; k < RD_NS; ++k) scal.write(rd_scal_index(g, ib, grp, k));
            for (int k = 0; k < walk_blocks(g); ++k)
                for (int c = 0; c < RD_NS; ++c) scal.read((size_t)k * RD_NS + (size_t)c);
            std::printf("reach sw=%zu sr=%zu sunwritten=%zu sdup=%zu slen=%zu outside=%d\n", scal.wmax, scal.rmax,
                        scal.unwritten, scal.dup, scal.len(), scal.outside ? 1 : 0);
        }
    }
    return 0;
}
