// CPU driver of the dual certificate's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_dual_geo.h) for tests/test_dual_geo.py.  One query per input line,
// `<what> <m> <n> <side>`:
//   geo     the grid and the buffer sizes
//   cover   walks the rows as the kernels' lanes do and the columns as their chunk loops do
//   reach   walks every index the walking kernels write and the finishing kernels read
// Per query it prints one line:
//   geo nib= ng= nslot= R= S= stride= part= blocks= scratch_dev= scratch_host=   (class 2, every array wanted)
//   cover rmin=<fewest (row block, thread) owners of a row i < m> rmax=<most> min=<fewest (group, chunk,
//         column-in-chunk) owners of a column j < n> max=<most> broke=<walks ended by j0 >= n> idle=<chunks not walked
//         after such an end> first=<1 when every group's first column is below n>
//   reach wmax=<largest transform partial written> rmax=<largest read> unwritten= dup= len= outside=
//         ewmax=<largest evaluation partial written> ermax=<largest read> eunwritten= edup= elen=
//   <what> refused     for a side outside {0, 1}
// The first line of the output is
//   limits TR= TC= APD_WAVES= DU_CPG= EVALPART=<bytes of a DuEvalPart>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_dual_geo.h"

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d DU_CPG=%d EVALPART=%zu\n", TR, TC, APD_WAVES, DU_CPG, sizeof(DuEvalPart));
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
                        du_eval_blocks(g), du_scratch_bytes(g, 2, true, true, false, false, false, false),
                        du_scratch_bytes(g, 2, true, false, true, true, true, true));
        } else if (what == "cover") {
            // rows: thread tid of row block ib owns row ib*TR + tid when that is below m
            std::vector<int> rown((size_t)m, 0);
            for (int ib = 0; ib < g.nib; ++ib)
                for (int tid = 0; tid < TR; ++tid) {
                    const int i = ib * TR + tid;
                    if (i < m) ++rown[(size_t)i];
                }
            // columns do not depend on the row block: one wave's walk per column group
            std::vector<int> owners((size_t)n, 0);
            long long broke = 0, idle = 0;
            int first = 1;
            for (int grp = 0; grp < g.ng; ++grp) {
                if (du_chunk_col(grp, 0) >= n) first = 0;   // k_du_rows starts its arg max there
                for (int ch = 0; ch < DU_CPG; ++ch) {
                    const int j0 = du_chunk_col(grp, ch);
                    if (j0 >= n) {   // the kernels: if (j0 >= g.n) break;
                        ++broke;
                        idle += DU_CPG - ch;
                        break;
                    }
                    for (int cc = 0; cc < TC; ++cc)
                        if (j0 + cc < n) ++owners[(size_t)(j0 + cc)];
                }
            }
            int lo = 1 << 30, hi = 0, rlo = 1 << 30, rhi = 0;
            for (int v : owners) {
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            for (int v : rown) {
                rlo = v < rlo ? v : rlo;
                rhi = v > rhi ? v : rhi;
            }
            std::printf("cover rmin=%d rmax=%d min=%d max=%d broke=%lld idle=%lld first=%d\n", rlo, rhi, lo, hi, broke, idle,
                        first);
        } else if (what == "reach") {
            const size_t len = du_part_len(g);
            std::vector<unsigned char> written(len, 0);
            size_t wmax = 0, rmax = 0, dup = 0, unwritten = 0;
            bool outside = false;
            auto write = [&](size_t idx) {
                wmax = idx > wmax ? idx : wmax;
                if (idx >= len) {
                    outside = true;
                    return;
                }
                dup += written[idx];
                written[idx] = 1;
            };
            if (side == 0) {
                // k_du_rows: the lane of row i < m of group grp stores its (max, arg max)
                for (int grp = 0; grp < g.ng; ++grp)
                    for (int i = 0; i < m; ++i) write(du_part_index(g, grp, i));
            } else {
                // k_du_cols: wave `slot` stores the maxima of the columns below n of every chunk it walks
                for (int slot = 0; slot < g.nslot; ++slot)
                    for (int grp = 0; grp < g.ng; ++grp)
                        for (int ch = 0; ch < DU_CPG; ++ch) {
                            const int j0 = du_chunk_col(grp, ch);
                            if (j0 >= n) break;
                            for (int cc = 0; cc < TC; ++cc)
                                if (j0 + cc < n) write(du_part_index(g, slot, j0 + cc));
                        }
            }
            // k_du_fin: S partials du_part_index(g, s, r)
            const int R = du_out_rows(g), S = du_part_count(g);
            for (int r = 0; r < R; ++r)
                for (int s = 0; s < S; ++s) {
                    const size_t idx = du_part_index(g, s, r);
                    rmax = idx > rmax ? idx : rmax;
                    if (idx >= len) outside = true;
                    else if (!written[idx]) ++unwritten;
                }
            // k_du_eval: workgroup (ib, grp) stores part[du_eval_index]; k_du_last reads 0 .. du_eval_blocks - 1
            const size_t elen = (size_t)du_eval_blocks(g);
            std::vector<unsigned char> ew(elen, 0);
            size_t ewmax = 0, edup = 0, eunwritten = 0;
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ib = 0; ib < g.nib; ++ib) {
                    const size_t idx = (size_t)du_eval_index(g, ib, grp);
                    ewmax = idx > ewmax ? idx : ewmax;
                    if (idx >= elen) {
                        outside = true;
                        continue;
                    }
                    edup += ew[idx];
                    ew[idx] = 1;
                }
            for (size_t k = 0; k < elen; ++k)
                if (!ew[k]) ++eunwritten;
            std::printf("reach wmax=%zu rmax=%zu unwritten=%zu dup=%zu len=%zu outside=%d ewmax=%zu ermax=%zu eunwritten=%zu "
                        "edup=%zu elen=%zu\n", wmax, rmax, unwritten, dup, len, outside ? 1 : 0, ewmax, elen - 1, eunwritten,
                        edup, elen);
        }
    }
    return 0;
}
