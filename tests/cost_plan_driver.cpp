// CPU driver of the point-cloud cost's host-clean header (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_cost_plan.h)
// for tests/test_cost_plan.py.  One query per input line:
//   check <metric> <dim> <m> <n> <scale> <xs> <ys>    xs, ys: ok | null | nan | inf (the last coordinate is the bad one)
//   scaleok <largest>
//   cover <m> <n> <rpl>                               walks the geometry as the build kernels do
//   rpl <m> <d> <aligned16> <IPD_COST_STORE value or ->
//   entry <metric> <d> <x_0 .. x_d-1> <y_0 .. y_d-1>  (hexadecimal floating point)
// Per query it prints one line:
//   check <NAME> limit=<0|1>
//   scaleok <0|1>
//   cover min=<fewest visits of an entry> max=<most> outside=<visits outside m x n> nib= njg= reps= waves=<waves with rows>
//   rpl <1|2>
//   entry <value, hexadecimal floating point>
// The first line of the output is
//   limits IPD_COST_DIM_MAX= IPD_APD_SIDE_MAX= COST_TC= COST_DT_MAX=
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_cost_plan.h"

static const double* make_coords(const std::string& how, size_t count, std::vector<double>* store) {
    if (how == "null") return nullptr;
    store->assign(count ? count : 1, 1.0);
    if (how == "nan") store->back() = std::numeric_limits<double>::quiet_NaN();
    if (how == "inf") store->back() = -std::numeric_limits<double>::infinity();
    return store->data();
}

int main() {
    std::printf("limits IPD_COST_DIM_MAX=%d IPD_APD_SIDE_MAX=%d COST_TC=%d COST_DT_MAX=%d\n", IPD_COST_DIM_MAX,
                IPD_APD_SIDE_MAX, COST_TC, COST_DT_MAX);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "check") {
            int metric = 0, dim = 0, scale = 0;
            long long m = 0, n = 0;
            std::string hx, hy;
            in >> metric >> dim >> m >> n >> scale >> hx >> hy;
            if (!in) continue;
            // the arrays are as long as a spec inside the limits needs (a spec outside is refused before they are read)
            const bool sane = dim >= 1 && dim <= IPD_COST_DIM_MAX && m >= 1 && n >= 1 && m <= IPD_APD_SIDE_MAX &&
                              n <= IPD_APD_SIDE_MAX;
            std::vector<double> sx, sy;
            const double* xs = make_coords(hx, sane ? (size_t)m * dim : 1, &sx);
            const double* ys = make_coords(hy, sane ? (size_t)n * dim : 1, &sy);
            const CostCheck ck = cost_spec_check(metric, dim, m, n, xs, ys, scale);
            std::printf("check %s limit=%d\n", COST_CHECK_NAMES[ck], ck == COST_SHAPE ? 1 : 0);
        } else if (what == "scaleok") {
            std::string v;
            in >> v;
            const double x = v == "nan" ? std::numeric_limits<double>::quiet_NaN()
                             : v == "inf" ? std::numeric_limits<double>::infinity()
                                          : std::strtod(v.c_str(), nullptr);
            std::printf("scaleok %d\n", cost_scale_ok(x) ? 1 : 0);
        } else if (what == "cover") {
            int m = 0, n = 0, rpl = 0;
            in >> m >> n >> rpl;
            if (!in) continue;
            const CostGeo g = cost_geo(m, n, rpl);
            std::vector<int> seen((size_t)m * n, 0);
            long long outside = 0, waves = 0;
            for (int ib = 0; ib < g.nib; ++ib)
                for (int jg = 0; jg < g.njg; ++jg)
                    for (int wv = 0; wv < COST_WAVES; ++wv) {
                        if (jg == 0 && cost_lane_row(g, ib, wv, 0) < m) ++waves;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int i0 = cost_lane_row(g, ib, wv, lane);
                            if (!(i0 < m)) continue;   // the kernels' in_i: the lane's rpl rows are inside together
                            for (int rep = 0; rep < g.reps; ++rep) {
                                const int j0 = cost_step_col(g, jg, rep);
                                if (j0 >= n) break;
                                for (int jj = 0; jj < COST_TC; ++jj) {
                                    if (!(j0 + jj < n)) continue;
                                    for (int r = 0; r < rpl; ++r) {
                                        const int i = i0 + r, j = j0 + jj;
                                        if (i >= m || j >= n) ++outside;
                                        else ++seen[(size_t)j * m + i];
                                    }
                                }
                            }
                        }
                    }
            int lo = 1 << 30, hi = 0;
            for (int v : seen) {
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            std::printf("cover min=%d max=%d outside=%lld nib=%d njg=%d reps=%d waves=%lld\n", lo, hi, outside, g.nib,
                        g.njg, g.reps, waves);
        } else if (what == "rpl") {
            int m = 0, d = 0, aligned = 0;
            std::string sw;
            in >> m >> d >> aligned >> sw;
            if (!in) continue;
            std::printf("rpl %d\n", cost_rows_per_lane(m, d, aligned != 0, sw == "-" ? nullptr : sw.c_str()));
        } else if (what == "entry") {
            int metric = 0, d = 0;
            in >> metric >> d;
            if (!in || d < 1 || d > IPD_COST_DIM_MAX) continue;
            double x[IPD_COST_DIM_MAX], y[IPD_COST_DIM_MAX];
            std::string tok;
            bool ok = true;
            for (int k = 0; k < 2 * d && ok; ++k) {
                ok = bool(in >> tok);
                if (ok) (k < d ? x[k] : y[k - d]) = std::strtod(tok.c_str(), nullptr);
            }
            if (ok) std::printf("entry %a\n", cost_entry(metric, d, x, y));
        }
    }
    return 0;
}
