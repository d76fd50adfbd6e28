// CPU driver of the problem-level solvers' host decisions (codes_of_ipd_ssn_amg_method_amd/csrc/ipd_hybrid_plan.h)
// for tests/test_hybrid_plan.py.  One query per input line (floating-point values as C99 hex floats):
//   components <N> <norder> <root[0..N)> <order[0..norder)>
//   route      <n> <bigph> <N> <ndk> <root[0..N)> <dK[0..ndk)>        ndk is 0 (no T) or N
//   sharing    <kind: 0 plain, 1 AMG4POT first, 2 AMG4POT second> <has_step> <same> <no_donor>
//   pot        <epss> <sg> <sum> <z2> <vvv> <vz1>
// Per query it prints one line:
//   components err=<text with _ for blanks, or -> ncomp= blocks= sizes= p= r=          (lists: comma separated)
//   route connected= it_num= gather_qp= one_sided= maxnb= small_lds= large=<k:off:len:fnode:mask:isnsp,...> nodes=
//         boff= local= p=
//   sharing record= from=<none|prev_step|first_solve> count= system=
//   pot phi_e= w= tt= zeta2=
// The first line of the output is
//   limits HYBRID_N0= RES_MASK_MIN_ROWS= HYBRID_SMALL_LDS_OPTIN=
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "ipd_hybrid_plan.h"

static std::string list(const std::vector<int>& v) {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + std::to_string(v[i]);
    return s.empty() ? "-" : s;
}

static bool read_ints(std::istream& in, int cnt, std::vector<int>* v) {
    v->assign((size_t)(cnt > 0 ? cnt : 0), 0);
    for (int& x : *v) in >> x;
    return cnt >= 0 && (bool)in;
}

static bool read_double(std::istream& in, double* x) {   // (operator>> does not read hex floats)
    std::string s;
    if (!(in >> s)) return false;
    char* end = nullptr;
    *x = std::strtod(s.c_str(), &end);
    return end && *end == 0;
}

int main() {
    std::printf("limits HYBRID_N0=%d RES_MASK_MIN_ROWS=%d HYBRID_SMALL_LDS_OPTIN=%zu\n", HYBRID_N0, RES_MASK_MIN_ROWS,
                HYBRID_SMALL_LDS_OPTIN);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        bool ok = true;
        if (what == "components") {
            int N = 0, norder = 0;
            std::vector<int> root, order;
            in >> N >> norder;
            ok = in && read_ints(in, N, &root) && read_ints(in, norder, &order);
            if (ok) {
                Components cc;
                const CompError e = components_from_roots(root.data(), N, order.data(), norder, &cc);
                std::string text = e == COMP_OK ? "-" : comp_error_text(e);
                for (char& c : text)
                    if (c == ' ') c = '_';
                if (e != COMP_OK) cc = Components();
                std::printf("components err=%s ncomp=%d blocks=%s sizes=%s p=%s r=%s\n", text.c_str(), cc.ncomp,
                            list(cc.blocks).c_str(), list(cc.sizes).c_str(), list(cc.p).c_str(), list(cc.r).c_str());
            }
        } else if (what == "route") {
            int n = 0, bigph = 0, N = 0, ndk = 0;
            std::vector<int> root;
            in >> n >> bigph >> N >> ndk;
            ok = in && (ndk == 0 || ndk == N) && read_ints(in, N, &root);
            std::vector<double> dK((size_t)(ok ? ndk : 0));
            for (double& x : dK) ok = ok && read_double(in, &x);
            Components cc;
            ok = ok && components_from_roots(root.data(), N, nullptr, 0, &cc) == COMP_OK;
            if (ok) {
                const HybridRoute rt = plan_route(cc, n, bigph != 0);
                std::string large;
                for (const LargeComponent& c : rt.large) {
                    const int isnsp = isnsp_of_dk(ndk ? dK.data() : nullptr, cc.p.data() + c.off, c.len);
                    large += (large.empty() ? "" : ",") + std::to_string(c.k) + ":" + std::to_string(c.off) + ":" +
                             std::to_string(c.len) + ":" + std::to_string(c.fnode) + ":" + std::to_string((int)c.mask) +
                             ":" + std::to_string(isnsp);
                }
                std::printf("route connected=%d it_num=%lld gather_qp=%d one_sided=%d maxnb=%d small_lds=%zu large=%s "
                            "nodes=%s boff=%s local=%s p=%s\n", (int)rt.connected, rt.it_num, (int)rt.gather_qp,
                            rt.one_sided, rt.maxnb, rt.small_lds, large.empty() ? "-" : large.c_str(),
                            list(rt.nodes).c_str(), list(rt.boff).c_str(), list(rt.local).c_str(), list(cc.p).c_str());
            }
        } else if (what == "sharing") {
            int kind = 0, has_step = 0, same = 0, no_donor = 0;
            in >> kind >> has_step >> same >> no_donor;
            ok = in && kind >= 0 && kind <= 2;
            if (ok) {
                const Sharing s = sharing_rule((HybridCallKind)kind, has_step != 0, same != 0, no_donor != 0);
                static const char* const FROM[] = {"none", "prev_step", "first_solve"};
                std::printf("sharing record=%d from=%s count=%d system=%d\n", (int)s.record, FROM[s.from], (int)s.count,
                            (int)s.system);
            }
        } else if (what == "pot") {
            double epss, sg, sum, z2, vvv, vz1;
            ok = read_double(in, &epss) && read_double(in, &sg) && read_double(in, &sum) && read_double(in, &z2) &&
                 read_double(in, &vvv) && read_double(in, &vz1);
            if (ok) {
                const double phi_e = pot_phi_e(epss, sg, sum);
                std::printf("pot phi_e=%a w=%a tt=%a zeta2=%a\n", phi_e, pot_w_coeff(sg, phi_e, z2),
                            pot_tt(sg, phi_e, vvv), pot_zeta2(z2, sg, vz1, phi_e));
            }
        } else
            ok = false;
        if (!ok) {
            std::fprintf(stderr, "bad query: %.200s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
