// CPU driver of the point-position gradient's host-clean geometry header
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_point_grad_geo.h) for tests/test_point_grad_geo.py.  One query per line:
//   geo <m> <n> <d> <side>      the grid, the passes and the buffer sizes
//   cover <m> <n> <d> <side>    walks the components as the launcher's pass loop does
//   reach <m> <n> <d> <side>    walks every index the walking kernel writes and the finishing kernel reads
//   h <metric> <d> <divide> <denom> <side> <x_0 .. x_d-1> <y_0 .. y_d-1>
//                               the d weights of one pair from the header's scalar code; denom and the coordinates
//                               are the 16 hex digits of their bits
// Per query it prints one line:
//   geo nib= ng= nslot= npass= reads= R= S= stride= plane= part= rec= scratch_dev= scratch_host= scratch_host_spec=
//   cover cmin=<fewest passes owning a component> cmax=<most> kcmax=<most components of a pass> tail=<of the last pass>
//   reach wmax= rmax= unwritten= dup= len= outside= recw=<largest record index written> recdup= reclen=
//   h kink=<0|1> w=<hex bits of weight 0> ... (d of them)
//   <what> refused     for a side outside {0, 1}, d outside [1, IPD_COST_DIM_MAX] or a metric outside [1, 4]
// (Built with -ffp-contract=off as the library: multiply and add stay separate whatever the host's -march.)
// The first line of the output is
//   limits TR= TC= APD_WAVES= WK_CPG= PG_KC= PG_NC= PG_DT_MAX= PG_REC= PG_STATS_DOUBLES= DIM_MAX=
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "geo_buf.h"
#include "ipd_point_grad_geo.h"

static double from_hex(const std::string& s) {
    const uint64_t b = std::strtoull(s.c_str(), nullptr, 16);
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}
static uint64_t to_bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main() {
    std::printf("limits TR=%d TC=%d APD_WAVES=%d WK_CPG=%d PG_KC=%d PG_NC=%d PG_DT_MAX=%d PG_REC=%d PG_STATS_DOUBLES=%d DIM_MAX=%d\n",
                TR, TC, APD_WAVES, WK_CPG, PG_KC, PG_NC, PG_DT_MAX, PG_REC, PG_STATS_DOUBLES, IPD_COST_DIM_MAX);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "h") {
            int metric = 0, d = 0, divide = 0, side = 0;
            std::string tok;
            in >> metric >> d >> divide >> tok >> side;
            if (metric < 1 || metric > 4 || d < 1 || d > IPD_COST_DIM_MAX || (side != 0 && side != 1)) {
                std::printf("h refused\n");
                continue;
            }
            const double denom = from_hex(tok);
            std::vector<double> x((size_t)d), y((size_t)d);
            for (int k = 0; k < d; ++k) {
                in >> tok;
                x[(size_t)k] = from_hex(tok);
            }
            for (int k = 0; k < d; ++k) {
                in >> tok;
                y[(size_t)k] = from_hex(tok);
            }
            int kink = 0;
            std::string out;
            for (int k = 0; k < d; ++k) {
                char buf[32];
                std::snprintf(buf, sizeof buf, " %016" PRIx64,
                              to_bits(pg_weight(metric, d, x.data(), y.data(), k, divide, denom, side, &kink)));
                out += buf;
            }
            std::printf("h kink=%d w=%s\n", kink, out.c_str() + 1);
            continue;
        }
        int m = 0, n = 0, d = 0, side = 0;
        if (!(in >> m >> n >> d >> side) || m < 1 || n < 1) continue;
        if ((side != 0 && side != 1) || d < 1 || d > IPD_COST_DIM_MAX) {   // what the ABI refuses
            std::printf("%s refused\n", what.c_str());
            continue;
        }
        const PgGeo g = pg_make_geo(m, n, d, side);
        if (what == "geo") {
            std::printf("geo nib=%d ng=%d nslot=%d npass=%d reads=%d R=%d S=%d stride=%zu plane=%zu part=%zu rec=%zu "
                        "scratch_dev=%zu scratch_host=%zu scratch_host_spec=%zu\n",
                        g.nib, g.ng, g.nslot, g.npass, pg_x_reads(g), pg_out_rows(g), pg_part_count(g), pg_part_stride(g),
                        pg_plane_len(g), pg_part_len(g), pg_rec_len(g), pg_scratch_bytes(g, false, false, true),
                        pg_scratch_bytes(g, true, true, true), pg_scratch_bytes(g, true, true, false));
        } else if (what == "cover") {
            std::vector<int> comp((size_t)d, 0);
            int kcmax = 0, tail = 0;
            for (int p = 0; p < g.npass; ++p) {
                const int kc = pg_pass_kc(g, p);
                kcmax = kc > kcmax ? kc : kcmax;
                tail = kc;
                for (int c = 0; c < kc; ++c) {
                    const int cc = pg_pass_c0(p) + c;
                    if (cc >= 0 && cc < d) ++comp[(size_t)cc];
                    else kcmax = 1 << 20;   // a component outside G
                }
            }
            int clo = 1 << 30, chi = 0;
            for (int v : comp) {
                clo = v < clo ? v : clo;
                chi = v > chi ? v : chi;
            }
            std::printf("cover cmin=%d cmax=%d kcmax=%d tail=%d\n", clo, chi, kcmax, tail);
        } else if (what == "reach") {
            // pass 0 of PG_KC components with the mass and the counts: the fullest the buffers get
            Buf part(pg_part_len(g)), rec(pg_rec_len(g));
            for (int grp = 0; grp < g.ng; ++grp)
                for (int ib = 0; ib < g.nib; ++ib)
                    for (int c = 0; c < PG_REC; ++c) rec.write(walk_block_index<size_t>(g, ib, grp) * PG_REC + (size_t)c);
            if (side == 0) {
                // lane of row i < m of group grp stores its PG_NC accumulators
                for (int grp = 0; grp < g.ng; ++grp)
                    for (int c = 0; c < PG_NC; ++c)
                        for (int i = 0; i < m; ++i) part.write(pg_part_index(g, grp, c, i));
            } else {
                // wave `slot` stores the sums of the columns below n of every chunk it walks
                for (int slot = 0; slot < g.nslot; ++slot)
                    for (int grp = 0; grp < g.ng; ++grp)
                        for (int ch = 0; ch < WK_CPG; ++ch) {
                            const int j0 = walk_chunk_col(grp, ch);
                            if (j0 >= n) break;
                            for (int cc = 0; cc < TC; ++cc)
                                if (j0 + cc < n)
                                    for (int c = 0; c < PG_NC; ++c) part.write(pg_part_index(g, slot, c, j0 + cc));
                        }
            }
            // k_pg_fin: S partials from pg_part_index(g, 0, c, r) at stride pg_part_stride(g)
            const int R = pg_out_rows(g), S = pg_part_count(g);
            for (int c = 0; c < PG_NC; ++c)
                for (int r = 0; r < R; ++r)
                    for (int s = 0; s < S; ++s) part.read(pg_part_index(g, 0, c, r) + (size_t)s * pg_part_stride(g));
            for (size_t b = 0; b < (size_t)walk_blocks(g) * PG_REC; ++b) rec.read(b);
            std::printf("reach wmax=%zu rmax=%zu unwritten=%zu dup=%zu len=%zu outside=%d recw=%zu recdup=%zu reclen=%zu "
                        "recunwritten=%zu\n",
                        part.wmax, part.rmax, part.unwritten, part.dup, part.len(), part.outside || rec.outside ? 1 : 0,
                        rec.wmax, rec.dup, rec.len(), rec.unwritten);
        }
    }
    return 0;
}
