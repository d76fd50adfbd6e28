// CPU driver of the plan products' host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_plan_apply_geo.h) for tests/test_plan_apply_geo.py.  One query per
// input line, `<what> <m> <n> <k> <side>`:
//   geo     the grid, the passes and the buffer sizes
//   cover   walks the components as the launcher's pass loop does (the columns: tests/walk_geo_driver.cpp)
//   reach   walks every index the walking kernels write and the finishing kernel reads of the partial buffer
// Per query it prints one line:
//   geo nib= ng= nslot= npass= R= S= stride= part= scratch_dev= scratch_host=
//   cover cmin=<fewest passes owning a component> cmax=<most> kcmax=<most components of a pass> tail=<components of
//         the last pass>
//   reach wmax=<largest index written> rmax=<largest index read> unwritten=<indices read by the finishing kernel
//         that no walking kernel writes in a pass of PA_KC components with the mass> dup=<indices written twice> len=
//   <what> refused     for a side outside {0, 1} or k outside [1, PA_KMAX]
// The first line of the output is
//   limits TR= TC= APD_WAVES= PA_KMAX= PA_KC= PA_NC= WK_CPG=
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "geo_buf.h"
#include "ipd_plan_apply_geo.h"

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d PA_KMAX=%d PA_KC=%d PA_NC=%d WK_CPG=%d\n", TR, TC, APD_WAVES, PA_KMAX,
                PA_KC, PA_NC, WK_CPG);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        int m = 0, n = 0, k = 0, side = 0;
        if (!(in >> what >> m >> n >> k >> side) || m < 1 || n < 1) continue;
        if ((side != 0 && side != 1) || k < 1 || k > PA_KMAX) {   // what the ABI refuses
            std::printf("%s refused\n", what.c_str());
            continue;
        }
        const PaGeo g = pa_make_geo(m, n, k, side);
        if (what == "geo") {
            std::printf("geo nib=%d ng=%d nslot=%d npass=%d R=%d S=%d stride=%zu part=%zu scratch_dev=%zu scratch_host=%zu\n",
                        g.nib, g.ng, g.nslot, g.npass, pa_out_rows(g), pa_part_count(g), pa_part_stride(g),
                        pa_part_len(g), pa_scratch_bytes(g, true, false, false), pa_scratch_bytes(g, false, true, true));
        } else if (what == "cover") {
            std::vector<int> comp((size_t)k, 0);
            int kcmax = 0, tail = 0;
            for (int p = 0; p < g.npass; ++p) {
                const int kc = pa_pass_kc(g, p);
                kcmax = kc > kcmax ? kc : kcmax;
                tail = kc;
                for (int c = 0; c < kc; ++c) {
                    const int cc = pa_pass_c0(p) + c;
                    if (cc >= 0 && cc < k) ++comp[(size_t)cc];
                    else kcmax = 1 << 20;   // a component outside B
                }
            }
            int clo = 1 << 30, chi = 0;
            for (int v : comp) {
                clo = v < clo ? v : clo;
                chi = v > chi ? v : chi;
            }
            std::printf("cover cmin=%d cmax=%d kcmax=%d tail=%d\n", clo, chi, kcmax, tail);
        } else if (what == "reach") {
            // one pass of PA_KC components with the mass: the fullest the buffer gets
            Buf part(pa_part_len(g));
            if (side == 0) {
                // k_pa_rows: lane of row i < m of group grp stores its PA_NC accumulators
                for (int grp = 0; grp < g.ng; ++grp)
                    for (int c = 0; c < PA_NC; ++c)
                        for (int i = 0; i < m; ++i) part.write(pa_part_index(g, grp, c, i));
            } else {
                // k_pa_cols: wave `slot` stores the sums of the columns below n of every chunk it walks
                for (int slot = 0; slot < g.nslot; ++slot)
                    for (int grp = 0; grp < g.ng; ++grp)
                        for (int ch = 0; ch < WK_CPG; ++ch) {
                            const int j0 = walk_chunk_col(grp, ch);
                            if (j0 >= n) break;
                            for (int cc = 0; cc < TC; ++cc)
                                if (j0 + cc < n)
                                    for (int c = 0; c < PA_NC; ++c) part.write(pa_part_index(g, slot, c, j0 + cc));
                        }
            }
            // k_pa_fin: S partials from pa_part_index(g, 0, c, r) at stride pa_part_stride(g)
            const int R = pa_out_rows(g), S = pa_part_count(g);
            for (int c = 0; c < PA_NC; ++c)
                for (int r = 0; r < R; ++r)
                    for (int s = 0; s < S; ++s) part.read(pa_part_index(g, 0, c, r) + (size_t)s * pa_part_stride(g));
            std::printf("reach wmax=%zu rmax=%zu unwritten=%zu dup=%zu len=%zu outside=%d\n", part.wmax, part.rmax,
                        part.unwritten, part.dup, part.len(), part.outside ? 1 : 0);
        }
    }
    return 0;
}
