// CPU driver of the column-group walk's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_walk_geo.h) for tests/test_walk_geo.py.  One query per input line,
// `<what> <m> <n>`:
//   geo     the grid and the sizes of the partial layouts
//   cover   walks the rows as the kernels' lanes do and the columns as their chunk loops do
//   reach   walks every index of the row, column and workgroup layouts as the walking kernels write them and the
//           finishing kernels read them
// Per query it prints one line:
//   geo nib= ng= nslot= rows= cols= blocks=
//   cover rmin=<fewest (row block, thread) owners of a row i < m> rmax=<most> min=<fewest (group, chunk,
//         column-in-chunk) owners of a column j < n> max=<most> broke=<walks ended by j0 >= n> idle=<chunks not walked
//         after such an end> first=<1 when every group's first column is below n>
//   reach rw=<largest row partial written> rr=<largest read> runwritten= rdup= rlen=   the same with c (column
//         partials) and b (workgroup records); outside=
// The first line of the output is
//   limits TR= TC= APD_WAVES= WK_CPG=
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "geo_buf.h"
#include "ipd_walk_geo.h"

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d WK_CPG=%d\n", TR, TC, APD_WAVES, WK_CPG);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int m = 0, n = 0;
        if (!(in >> what >> m >> n) || m < 1 || n < 1) continue;
        const WalkGeo g = walk_make_geo(m, n);
        if (what == "geo") {
            std::printf("geo nib=%d ng=%d nslot=%d rows=%zu cols=%zu blocks=%d\n", g.nib, g.ng, g.nslot,
                        walk_row_part_len(g), walk_col_part_len(g), walk_blocks(g));
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
                if (walk_chunk_col(grp, 0) >= n) first = 0;   // k_du_rows starts its arg max there
                for (int ch = 0; ch < WK_CPG; ++ch) {
                    const int j0 = walk_chunk_col(grp, ch);
                    if (j0 >= n) {   // the kernels: if (j0 >= g.n) break;
                        ++broke;
                        idle += WK_CPG - ch;
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
            Buf rows(walk_row_part_len(g)), cols(walk_col_part_len(g)), blks((size_t)walk_blocks(g));
            // a walking kernel: workgroup (ib, grp), wave wv, lane of row i
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ib = 0; ib < g.nib; ++ib) {
                    for (int tid = 0; tid < TR; ++tid) {
                        const int i = ib * TR + tid;
                        if (i < m) rows.write(walk_row_part_index(g, grp, i));
                    }
                    for (int wv = 0; wv < APD_WAVES; ++wv)
                        for (int ch = 0; ch < WK_CPG; ++ch) {
                            const int j0 = walk_chunk_col(grp, ch);
                            if (j0 >= n) break;
                            for (int cc = 0; cc < TC; ++cc)   // lanes 0 .. 15, each its own column of the chunk
                                if (j0 + cc < n) cols.write(walk_col_part_index(g, walk_slot(ib, wv), j0 + cc));
                        }
                    blks.write((size_t)walk_block_index(g, ib, grp));
                    if (walk_block_index<size_t>(g, ib, grp) != (size_t)walk_block_index(g, ib, grp)) blks.outside = true;
                }
            // a finishing kernel: a row's ng partials at stride m, a column's nslot partials at stride n, the
            // workgroups' records 0 .. blocks - 1
            for (int i = 0; i < m; ++i)
                for (int s = 0; s < g.ng; ++s) rows.read((size_t)i + (size_t)s * (size_t)m);
            for (int j = 0; j < n; ++j)
                for (int s = 0; s < g.nslot; ++s) cols.read((size_t)j + (size_t)s * (size_t)n);
            for (int k = 0; k < walk_blocks(g); ++k) blks.read((size_t)k);
            std::printf("reach rw=%zu rr=%zu runwritten=%zu rdup=%zu rlen=%zu cw=%zu cr=%zu cunwritten=%zu cdup=%zu clen=%zu "
                        "bw=%zu br=%zu bunwritten=%zu bdup=%zu blen=%zu outside=%d\n",
                        rows.wmax, rows.rmax, rows.unwritten, rows.dup, rows.len(), cols.wmax, cols.rmax, cols.unwritten,
                        cols.dup, cols.len(), blks.wmax, blks.rmax, blks.unwritten, blks.dup, blks.len(),
                        (rows.outside || cols.outside || blks.outside) ? 1 : 0);
        }
    }
    return 0;
}
