// Every host decision of the problem-level solvers (Hybrid_AMG.m:27-107, components.m:32-55,
// Class2/AMG4POT.m:31-54), host-clean: the standard library and ipd_limits.h only, so that
// tests/hybrid_plan_driver.cpp runs each rule at its boundaries with a plain C++ compiler.  The executors
// (ipd_components.hip, ipd_hybrid.hip, ipd_pot.hip) take what these functions return and decide nothing themselves.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "ipd_limits.h"

// ---------------------------------------------------------------------------------------------------------------
// connected components                                                                       (components.m:32-55)
// ---------------------------------------------------------------------------------------------------------------
struct Components {
    int ncomp = 0;
    std::vector<int> blocks;  // component of every node (numbered by smallest member)
    std::vector<int> sizes;
    std::vector<int> p;       // nodes grouped by component, ascending inside a component
    std::vector<int> r;       // boundaries, ncomp+1
};

enum CompError { COMP_OK = 0, COMP_BAD_ROOT, COMP_ORDER_LENGTH, COMP_ORDER_ENTRY };
// (COMP_BAD_ROOT is a numeric failure of the union-find, the other two are argument errors)
inline const char* comp_error_text(CompError e) {
    switch (e) {
        case COMP_BAD_ROOT: return "components: a node does not point at the smallest member of its tree";
        case COMP_ORDER_LENGTH: return "component order: as many entries as there are components expected";
        case COMP_ORDER_ENTRY: return "component order: entries must be the smallest members of distinct components";
        default: return "";
    }
}

// root[i]: the smallest member of i's tree (what k_cc_flatten leaves).  Components are numbered by smallest
// member and members ascend inside a component.
// An injected visiting order (SURVEY A-9: MATLAB's dmperm order is undocumented, so a recorded one can be
// replayed; norder == 0: none): component k of the result is the one whose smallest member is order[k].
// Members stay ascending inside a component (F side first).  The order only moves info(2), the loop order
// and with it the order in which rand is consumed.
inline CompError components_from_roots(const int* root, int N, const int* order, int norder, Components* out) {
    out->blocks.assign((size_t)N, 0);
    std::vector<int> cid((size_t)N, -1);
    int nc = 0;
    for (int i = 0; i < N; ++i)
        if (root[i] == i) cid[(size_t)i] = nc++;  // roots ascend == smallest members ascend
    out->ncomp = nc;
    out->sizes.assign((size_t)nc, 0);
    for (int i = 0; i < N; ++i) {
        if (!(root[i] >= 0 && root[i] <= i && cid[(size_t)root[i]] >= 0)) return COMP_BAD_ROOT;
        out->blocks[(size_t)i] = cid[(size_t)root[i]];
        out->sizes[(size_t)out->blocks[(size_t)i]]++;
    }
    if (norder) {
        if (norder != nc) return COMP_ORDER_LENGTH;
        std::vector<int> newid((size_t)nc, -1), sizes((size_t)nc, 0);
        for (int k = 0; k < nc; ++k) {
            const int sm = order[k];
            if (!(sm >= 0 && sm < N && root[sm] == sm && newid[(size_t)cid[(size_t)sm]] < 0)) return COMP_ORDER_ENTRY;
            newid[(size_t)cid[(size_t)sm]] = k;
        }
        for (int c = 0; c < nc; ++c) sizes[(size_t)newid[(size_t)c]] = out->sizes[(size_t)c];
        out->sizes = sizes;
        for (int i = 0; i < N; ++i) out->blocks[(size_t)i] = newid[(size_t)out->blocks[(size_t)i]];
    }
    out->r.assign((size_t)nc + 1, 0);
    for (int c = 0; c < nc; ++c) out->r[(size_t)c + 1] = out->r[(size_t)c] + out->sizes[(size_t)c];
    out->p.assign((size_t)N, 0);
    std::vector<int> cur(out->r.begin(), out->r.end() - 1);
    for (int i = 0; i < N; ++i) out->p[(size_t)cur[(size_t)out->blocks[(size_t)i]]++] = i;
    return COMP_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Hybrid_AMG's route                                                                        (Hybrid_AMG.m:30-107)
// ---------------------------------------------------------------------------------------------------------------
struct LargeComponent {   // one Class_AMG solve: the whole system when connected, else a component beyond HYBRID_N0
    int k = 0;            // its number (it_num = k + 1 once it is solved, Hybrid_AMG.m:80)
    int off = 0, len = 0; // its nodes: cc.p[off .. off + len), ascending: F side first (quirk A-9)
    int fnode = 0;        // :68 sum(pk <= n): its F rows
    bool mask = false;    // level 1 is offered in mask form (amg_attach_maskop) with the component's p and q
};
struct HybridRoute {
    bool connected = false;              // :30 one component: Ae itself, no gather and no scatter
    std::vector<LargeComponent> large;   // in visiting order
    int one_sided = -1;                  // the first large component with fnode == 0 or == len (an error), or -1
    bool gather_qp = false;              // some component needs [q; p] in the order of the unknowns for its mask form
    // :85-91 the small components together: block b holds nodes[boff[b] .. boff[b+1]), local[i] is i's row in its block
    std::vector<int> nodes, boff, local;
    int maxnb = 0;
    size_t small_lds = 0;                // dynamic LDS bytes of k_small_blocks
    long long it_num = 0;                // info(2)
};

inline HybridRoute plan_route(const Components& cc, int n, bool bigph) {
    HybridRoute rt;
    const int M = (int)cc.p.size();
    rt.connected = cc.ncomp == 1;
    rt.boff.assign(1, 0);
    if (rt.connected) {                                                    // :30-48
        LargeComponent c;
        c.len = M;
        c.fnode = n;
        c.mask = bigph;
        rt.large.push_back(c);
        rt.it_num = 1;
        return rt;
    }
    rt.local.assign((size_t)M, 0);
    for (int k = 0; k < cc.ncomp; ++k) {
        const int off = cc.r[(size_t)k], len = cc.sizes[(size_t)k];
        if (len > HYBRID_N0) {                                             // :53
            LargeComponent c;
            c.k = k;
            c.off = off;
            c.len = len;
            for (int r = 0; r < len; ++r) c.fnode += cc.p[(size_t)(off + r)] < n;
            c.mask = bigph && len > RES_MASK_MIN_ROWS;
            rt.gather_qp = rt.gather_qp || c.mask;
            if (rt.one_sided < 0 && !(c.fnode > 0 && c.fnode < len)) rt.one_sided = k;
            rt.large.push_back(c);
            rt.it_num = k + 1;                                             // :80 (1-based)
        } else {                                                           // :85
            for (int r = 0; r < len; ++r) {
                rt.local[(size_t)cc.p[(size_t)(off + r)]] = r;
                rt.nodes.push_back(cc.p[(size_t)(off + r)]);
            }
            rt.boff.push_back((int)rt.nodes.size());
            rt.maxnb = std::max(rt.maxnb, len);
        }
    }
    rt.small_lds = hybrid_small_lds(rt.maxnb);
    return rt;
}

// :32-38 / :60-66  isnsp = 0 when dK sums to something over the component's nodes (ascending), else 1;
// hdK == NULL: T is absent, dK is zero
inline int isnsp_of_dk(const double* hdK, const int* idx, int cnt) {
    if (!hdK) return 1;
    double s = 0.0;
    for (int k = 0; k < cnt; ++k) s += hdK[idx[k]];
    return s != 0.0 ? 0 : 1;
}

// ---------------------------------------------------------------------------------------------------------------
// which setups share whose levels (row f3)
// ---------------------------------------------------------------------------------------------------------------
// A setup that is handed a donor hierarchy shares its rand-independent part (amg_setup's `donor`: levels 1-2), bit
// for bit the result of a full setup.  Two sources: the previous Newton step of a driver when it had this very system
// (StepDonors, `same`), and the first of AMG4POT's two solves for the second (Class2/AMG4POT.m:46-47, same Ae).
enum HybridCallKind { CALL_PLAIN = 0, CALL_POT_FIRST, CALL_POT_SECOND };
enum DonorSource { DONORS_NONE = 0, DONORS_PREV_STEP, DONORS_FIRST_SOLVE };
struct Sharing {
    bool record = false;              // keep this call's hierarchies (for the next step, or for the second solve)
    DonorSource from = DONORS_NONE;   // whose hierarchies its setups are offered, in visiting order
    bool count = false;               // count the setups that took a donor's levels in StepDonors::shared
    bool system = false;              // AMG4POT's two solves share Ae and the components (the first makes them)
};
// no_donor: IPD_NO_DONOR, which switches AMG4POT's sharing off (a plain call never looked at it)
inline Sharing sharing_rule(HybridCallKind kind, bool has_step, bool same, bool no_donor) {
    Sharing s;
    switch (kind) {
        case CALL_PLAIN:
            s.record = has_step;
            s.from = has_step && same ? DONORS_PREV_STEP : DONORS_NONE;
            s.count = has_step;
            break;
        case CALL_POT_FIRST:
            s.record = !no_donor;
            s.from = !no_donor && has_step && same ? DONORS_PREV_STEP : DONORS_NONE;
            s.count = s.from == DONORS_PREV_STEP;
            s.system = !no_donor;
            break;
        case CALL_POT_SECOND:
            s.from = no_donor ? DONORS_NONE : DONORS_FIRST_SOLVE;
            s.system = !no_donor;
            break;
    }
    return s;
}

// ---------------------------------------------------------------------------------------------------------------
// AMG4POT's Sherman-Morrison scalars, with the reference's operation order           (Class2/AMG4POT.m:31-54)
// ---------------------------------------------------------------------------------------------------------------
// sg = 1/tk, epss = bk1 (:31); sum = phi'*(s.*phi); z2 = z(end); vvv = v'*vv, vz1 = v'*zeta1
inline double pot_phi_e(double epss, double sg, double sum) { return epss + sg * sum; }              // :33
inline double pot_w_coeff(double sg, double phi_e, double z2) { return -(sg / phi_e * z2); }          // w = z1 + (.)*v
inline double pot_tt(double sg, double phi_e, double vvv) { return sg * sg / (phi_e - sg * sg * vvv); }   // :53
inline double pot_zeta2(double z2, double sg, double vz1, double phi_e) { return (z2 - sg * vz1) / phi_e; }   // :54
