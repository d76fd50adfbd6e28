// CPU driver of the primal certificate's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_round_geo.h) for tests/test_round_geo.py.  One query per input line,
// `<what> <m> <n>`:
//   geo     the grid, the buffer sizes and the scratch of a call
//   cover   walks the rows as the kernels' lanes do and the columns as their chunk loops do
//   reach   walks every index the walking kernel writes and the finishing and last kernels read
// Per query it prints one line:
//   geo nib= ng= nslot= rows= cols= blocks= scal= scratch=
//   cover rmin=<fewest (row block, thread) owners of a row i < m> rmax=<most> min=<fewest (group, chunk,
//         column-in-chunk) owners of a column j < n> max=<most> broke=<walks ended by j0 >= n> idle=<chunks not walked
//         after such an end>
//   reach rw=<largest row partial written> rr=<largest read> runwritten= rdup= rlen=
//         cw=<largest column partial written> cr=<largest read> cunwritten= cdup= clen=
//         sw=<largest scalar partial written> sr=<largest read> sunwritten= sdup= slen= outside=
// The first line of the output is
//   limits TR= TC= APD_WAVES= RD_CPG= RD_NS= RD_NVEC= RD_SCAL_PASSES= RD_RESULT_DOUBLES=
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_round_geo.h"

namespace {

struct Buf {
    std::vector<unsigned char> written;
    size_t wmax = 0, rmax = 0, dup = 0, unwritten = 0;
    bool outside = false;
    explicit Buf(size_t len) : written(len, 0) {}
    void write(size_t idx) {
        wmax = idx > wmax ? idx : wmax;
        if (idx >= written.size()) {
            outside = true;
            return;
        }
        dup += written[idx];
        written[idx] = 1;
    }
    void read(size_t idx) {
        rmax = idx > rmax ? idx : rmax;
        if (idx >= written.size())
            outside = true;
        else if (!written[idx])
            ++unwritten;
    }
};

}  // namespace

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d RD_CPG=%d RD_NS=%d RD_NVEC=%d RD_SCAL_PASSES=%d RD_RESULT_DOUBLES=%d\n",
                TR, TC, APD_WAVES, RD_CPG, RD_NS, RD_NVEC, RD_SCAL_PASSES, RD_RESULT_DOUBLES);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int m = 0, n = 0;
        if (!(in >> what >> m >> n) || m < 1 || n < 1) continue;
        const RdGeo g = rd_make_geo(m, n);
        if (what == "geo") {
            std::printf("geo nib=%d ng=%d nslot=%d rows=%zu cols=%zu blocks=%d scal=%zu scratch=%zu\n", g.nib, g.ng,
                        g.nslot, rd_row_len(g), rd_col_len(g), rd_blocks(g), rd_scal_len(g), round_scratch_bytes(g));
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
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ch = 0; ch < RD_CPG; ++ch) {
                    const int j0 = rd_chunk_col(grp, ch);
                    if (j0 >= n) {   // the kernel: if (j0 >= g.n) break;
                        ++broke;
                        idle += RD_CPG - ch;
                        break;
                    }
                    for (int cc = 0; cc < TC; ++cc)
                        if (j0 + cc < n) ++owners[(size_t)(j0 + cc)];
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
            std::printf("cover rmin=%d rmax=%d min=%d max=%d broke=%lld idle=%lld\n", rlo, rhi, lo, hi, broke, idle);
        } else if (what == "reach") {
            Buf rows(rd_row_len(g)), cols(rd_col_len(g)), scal(rd_scal_len(g));
            // k_rd_walk: workgroup (ib, grp), wave wv, lane of row i
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ib = 0; ib < g.nib; ++ib) {
                    for (int tid = 0; tid < TR; ++tid) {
                        const int i = ib * TR + tid;
                        if (i < m) rows.write(rd_row_index(g, grp, i));   // if (ROWS && in_i)
                    }
                    for (int wv = 0; wv < APD_WAVES; ++wv)
                        for (int ch = 0; ch < RD_CPG; ++ch) {
                            const int j0 = rd_chunk_col(grp, ch);
                            if (j0 >= n) break;
                            for (int cc = 0; cc < TC; ++cc)   // lanes 0 .. 15, each its own column of the chunk
                                if (j0 + cc < n) cols.write(rd_col_index(g, rd_slot(ib, wv), j0 + cc));
                        }
                    for (int k = 0; k < RD_NS; ++k) scal.write(rd_scal_index(g, ib, grp, k));
                }
            // k_rd_fin: a row's ng partials at stride m, a column's nslot partials at stride n
            for (int i = 0; i < m; ++i)
                for (int s = 0; s < g.ng; ++s) rows.read((size_t)i + (size_t)s * (size_t)m);
            for (int j = 0; j < n; ++j)
                for (int s = 0; s < g.nslot; ++s) cols.read((size_t)j + (size_t)s * (size_t)n);
            // k_rd_last: workgroup k's scalars at k*RD_NS + 0 .. RD_NS - 1
            for (int k = 0; k < rd_blocks(g); ++k)
                for (int c = 0; c < RD_NS; ++c) scal.read((size_t)k * RD_NS + (size_t)c);
            std::printf("reach rw=%zu rr=%zu runwritten=%zu rdup=%zu rlen=%zu cw=%zu cr=%zu cunwritten=%zu cdup=%zu clen=%zu "
                        "sw=%zu sr=%zu sunwritten=%zu sdup=%zu slen=%zu outside=%d\n",
                        rows.wmax, rows.rmax, rows.unwritten, rows.dup, rows.written.size(), cols.wmax, cols.rmax,
                        cols.unwritten, cols.dup, cols.written.size(), scal.wmax, scal.rmax, scal.unwritten, scal.dup,
                        scal.written.size(), (rows.outside || cols.outside || scal.outside) ? 1 : 0);
        }
    }
    return 0;
}
