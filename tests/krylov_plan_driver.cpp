// CPU driver of the host rules and the scalar step of the Krylov and block solves
// (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_krylov_plan.h, ipd_pcg_step.h) for tests/test_krylov_plan.py.
// The first line of the output is
//   limits <BT> <STAGE_MAX> <BLK_WMAX> <PCG_SMALL_MAXIT>
// then one answer line per input line:
//   width <n>                      -> <W>                    block_width, and the arm with_block_width takes for it
//   chunks <nrhs>                  -> <j0>,<ncol>,<W> ...
//   stage <len> <W>                -> <staged> <dyn bytes>
//   g3 <N> <num_cu>                -> <G3>
//   io <N> <W>                     -> <grid> <threads>
//   route <small_ok> <maxit>       -> <route>
//   opts null | <retol> <maxit> <precd>   -> <ok> <tol> <maxit>
//   resk <c> <maxit> <it>          -> <slot>
//   stride <maxit>                 -> <stride>
//   step <maxit> <tol> <d0> [<pq> <rw> <rwo>]...
//        -> first <it> <res> <stop> then per triple: | <alpha> <beta> <res> <it> <stop>
// Doubles go in and out as C99 hexadecimal floats (bit for bit).  The step runs on the record S[SC_N]; the
// functions over values must give the same bits (exit status 3 otherwise).
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "ipd_krylov_plan.h"
#include "ipd_pcg_step.h"

static double hex_in(std::istream& in) {
    std::string t;
    in >> t;
    return std::strtod(t.c_str(), nullptr);
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

int main() {
    std::printf("limits %d %d %d %d\n", BT, STAGE_MAX, BLK_WMAX, PCG_SMALL_MAXIT);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "width") {
            long long n;
            in >> n;
            int arm = 0;
            with_block_width(block_width(n), [&](auto Wc) { arm = decltype(Wc)::value; });
            if (arm != block_width(n)) return 3;
            std::printf("%d\n", arm);
        } else if (cmd == "chunks") {
            long long nrhs;
            in >> nrhs;
            block_chunks(nrhs, [](long long j0, int ncol, int W) { std::printf("%lld,%d,%d ", j0, ncol, W); });
            std::printf("\n");
        } else if (cmd == "stage") {
            long long len;
            int W;
            in >> len >> W;
            const BlockStage st = block_stage(len, W);
            std::printf("%d %zu\n", st.staged ? 1 : 0, st.dyn);
        } else if (cmd == "g3") {
            int N, cu;
            in >> N >> cu;
            std::printf("%d\n", krylov_g3(N, cu));
        } else if (cmd == "io") {
            long long N;
            int W;
            in >> N >> W;
            std::printf("%d %d\n", block_io_grid(N, W), BLK_IO_BT);
        } else if (cmd == "route") {
            int ok;
            long long maxit;
            in >> ok >> maxit;
            std::printf("%d\n", (int)pcg_route(ok != 0, maxit));
        } else if (cmd == "opts") {
            std::string first;
            in >> first;
            ipd_pcg_opts o;
            std::memset(&o, 0, sizeof o);
            const bool null = first == "null";
            if (!null) {
                long long mi;
                int pr;
                o.retol = std::strtod(first.c_str(), nullptr);
                in >> mi >> pr;
                o.maxit = mi;
                o.precd = pr;
            }
            double tol = -1.0;
            long long maxit = -1;
            const bool ok = pcg_opts_rule(null ? nullptr : &o, &tol, &maxit);
            std::printf("%d %a %lld\n", ok ? 1 : 0, tol, maxit);
        } else if (cmd == "resk") {
            long long c, maxit, it;
            in >> c >> maxit >> it;
            std::printf("%zu\n", pcg_resk_slot(c, maxit, it));
        } else if (cmd == "stride") {
            long long maxit;
            in >> maxit;
            std::printf("%lld\n", multi_hist_stride(maxit));
        } else if (cmd == "step") {
            double maxit;
            in >> maxit;
            const double tol = hex_in(in), d0 = hex_in(in);
            const double tol2 = tol * tol;   // as the launches form it
            double S[SC_N];
            for (double& v : S) v = -7.0;   // every field the step reads must have been written by it
            bool go = pcg_step<true>(S, d0, 0.0, maxit, tol2);
            if ((S[SC_STOP] == 0.0) != go || !same_bits(S[SC_RES], pcg_res(d0, d0)) || S[SC_BETA] != 0.0) return 3;
            std::printf("first %d %a %d", (int)S[SC_IT], S[SC_RES], go ? 0 : 1);
            std::string t;
            while (in >> t) {
                const double pq = std::strtod(t.c_str(), nullptr), rw = hex_in(in), rwo = hex_in(in);
                const double dold = S[SC_DNEW];
                pcg_step_alpha(S, pq);
                go = pcg_step<false>(S, rw, rwo, maxit, tol2);
                if ((S[SC_STOP] == 0.0) != go || !same_bits(S[SC_BETA], pcg_beta(rw, rwo, dold)) ||
                    !same_bits(S[SC_RES], pcg_res(rw, d0)) || !same_bits(S[SC_DOLD], dold) ||
                    !same_bits(S[SC_D0], d0) || !same_bits(S[SC_DNEW], rw))
                    return 3;
                std::printf(" | %a %a %a %d %d", S[SC_ALPHA], S[SC_BETA], S[SC_RES], (int)S[SC_IT], go ? 0 : 1);
            }
            std::printf("\n");
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
