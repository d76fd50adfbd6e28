// CPU driver of the dual certificate's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_dual_geo.h) for tests/test_dual_geo.py.  One query per input line,
// `<what> <m> <n> <side>`:
//   geo     the grid and the buffer sizes
//   reach   walks every index the walking kernels write and the finishing kernels read
// (the walk of the rows and the columns itself: tests/walk_geo_driver.cpp)
// Per query it prints one line:
//   geo nib= ng= nslot= R= S= stride= part= blocks= scratch_dev= scratch_host=   (class 2, every array wanted)
//   reach wmax=<largest transform partial written> rmax=<largest read> unwritten= dup= len= outside=
//         ewmax=<largest evaluation partial written> ermax=<largest read> eunwritten= edup= elen=
//   <what> refused     for a side outside {0, 1}
// The first line of the output is
//   limits TR= TC= APD_WAVES= WK_CPG= EVALPART=<bytes of a DuEvalPart>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "geo_buf.h"
#include "ipd_dual_geo.h"

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d WK_CPG=%d EVALPART=%zu\n", TR, TC, APD_WAVES, WK_CPG, sizeof(DuEvalPart));
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int m = 0, n = 0, side = 0;
        if (!(in >> what >> m >> n >> side) || m < 1 || n < 1) continue;
        if (side != 0 && side != 1) {
            std::printf("%s refused\n", what.c_str());
            continue;
        }
        const DuGeo g = du_make_geo(m, n, side);
        if (what == "geo") {
            std::printf("geo nib=%d ng=%d nslot=%d R=%d S=%d stride=%zu part=%zu blocks=%d scratch_dev=%zu scratch_host=%zu\n",
                        g.nib, g.ng, g.nslot, du_out_rows(g), du_part_count(g), du_part_stride(g), du_part_len(g),
                        walk_blocks(g), du_scratch_bytes(g, 2, true, true, false, false, false, false),
                        du_scratch_bytes(g, 2, true, false, true, true, true, true));
        } else if (what == "reach") {
            Buf part(du_part_len(g)), ev((size_t)walk_blocks(g));
            if (side == 0) {
                // k_du_rows: the lane of row i < m of group grp stores its (max, arg max)
                for (int grp = 0; grp < g.ng; ++grp)
                    for (int i = 0; i < m; ++i) part.write(du_part_index(g, grp, i));
            } else {
                // k_du_cols: wave `slot` stores the maxima of the columns below n of every chunk it walks
                for (int slot = 0; slot < g.nslot; ++slot)
                    for (int grp = 0; grp < g.ng; ++grp)
                        for (int ch = 0; ch < WK_CPG; ++ch) {
                            const int j0 = walk_chunk_col(grp, ch);
                            if (j0 >= n) break;
                            for (int cc = 0; cc < TC; ++cc)
                                if (j0 + cc < n) part.write(du_part_index(g, slot, j0 + cc));
                        }
            }
            // k_du_fin: S partials du_part_index(g, s, r)
            const int R = du_out_rows(g), S = du_part_count(g);
            for (int r = 0; r < R; ++r)
                for (int s = 0; s < S; ++s) part.read(du_part_index(g, s, r));
            // k_du_eval: workgroup (ib, grp) stores part[walk_block_index]; k_du_last reads 0 .. walk_blocks - 1
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ib = 0; ib < g.nib; ++ib) ev.write((size_t)walk_block_index(g, ib, grp));
            for (size_t k = 0; k < ev.len(); ++k) ev.read(k);
            std::printf("reach wmax=%zu rmax=%zu unwritten=%zu dup=%zu len=%zu outside=%d ewmax=%zu ermax=%zu eunwritten=%zu "
                        "edup=%zu elen=%zu\n", part.wmax, part.rmax, part.unwritten, part.dup, part.len(),
                        (part.outside || ev.outside) ? 1 : 0, ev.wmax, ev.rmax, ev.unwritten, ev.dup, ev.len());
        }
    }
    return 0;
}
