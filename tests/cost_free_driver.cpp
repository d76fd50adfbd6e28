// CPU driver of the matrix-free cost source (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_cost_plan.h: CostSrc,
// cost_src_entry, cost_free_check) for tests/test_cost_free_plan.py.  One query per input line:
//   check <dim>
//   matrix <metric> <dim> <m> <n> <scale> <m*dim coordinates of xs> <n*dim of ys>
//       coordinate-major (xs[i + k*m], ys[j + k*n]), hexadecimal floating point.  scale = 1 divides by the largest
//       entry of the unscaled matrix, which this driver finds with cost_src_entry as the build kernel's first pass
//       finds it on the device.
// Per query it prints one line:
//   check <OK|DIM> limit=<0|1> text=<the refusal names the limit: 0|1>
//   matrix <m*n entries, column-major (i + j*m), hexadecimal floating point>
// The first line of the output is
//   limits COST_FREE_DIM_MAX= COST_DT_MAX=
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_cost_plan.h"

int main() {
    std::printf("limits COST_FREE_DIM_MAX=%d COST_DT_MAX=%d\n", COST_FREE_DIM_MAX, COST_DT_MAX);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "check") {
            int dim = 0;
            in >> dim;
            if (!in) continue;
            const CostFreeCheck ck = cost_free_check(dim);
            const std::string limit = "[1, " + std::to_string(COST_FREE_DIM_MAX) + "]";
            std::printf("check %s limit=%d text=%d\n", ck == COST_FREE_OK ? "OK" : "DIM", ck == COST_FREE_OK ? 0 : 1,
                        std::strstr(COST_FREE_TEXT[COST_FREE_DIM], limit.c_str()) ? 1 : 0);
        } else if (what == "matrix") {
            int metric = 0, dim = 0, m = 0, n = 0, scale = 0;
            in >> metric >> dim >> m >> n >> scale;
            if (!in || cost_free_check(dim) != COST_FREE_OK || m < 1 || n < 1) continue;
            std::vector<double> xs((size_t)m * dim), ys((size_t)n * dim);
            std::string tok;
            bool ok = true;
            for (size_t t = 0; t < xs.size() + ys.size() && ok; ++t) {
                ok = bool(in >> tok);
                if (ok) (t < xs.size() ? xs[t] : ys[t - xs.size()]) = std::strtod(tok.c_str(), nullptr);
            }
            if (!ok) continue;
            CostSrc s{};
            s.xs = xs.data();
            s.ys = ys.data();
            s.m = m;
            s.n = n;
            s.dim = dim;
            s.metric = metric;
            if (scale) {
                double largest = cost_src_entry(s, 0, 0);
                for (int j = 0; j < n; ++j)
                    for (int i = 0; i < m; ++i) {
                        const double v = cost_src_entry(s, i, j);
                        largest = v > largest ? v : largest;
                    }
                s.divide = 1;
                s.denom = largest;
            }
            std::printf("matrix");
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < m; ++i) std::printf(" %a", cost_src_entry(s, i, j));
            std::printf("\n");
        }
    }
    return 0;
}
