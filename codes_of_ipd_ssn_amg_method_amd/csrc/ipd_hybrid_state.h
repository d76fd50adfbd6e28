// The problem-level solvers (Hybrid_AMG, AMG4POT, aug_PCG, PCG4POT, the dense Class 2 routes): the records they
// pass each other and the host functions that cross their units, grouped by the unit that defines them.  A kernel
// is launched only by the unit that defines it; another unit calls one of these functions.  Host-only.  The host
// decisions are in ipd_hybrid_plan.h (host-clean).
#pragma once

#include <functional>

#include "ipd_amg_internal.h"
#include "ipd_hybrid_plan.h"

// One Newton system on the device: H0 = A*S*A' with its active set, T's diagonal (NULL: none), p, q and the two
// scalars of  Ae = bk1*Q0^2 + (Q0*T*Q0 + Q0*H0*Q0)/tk,  Q0 = diag([q; -p])  (Hybrid_AMG.m:17-24)
struct NewtonSys {
    Csr H0;
    const double* tdiag = nullptr;
    const double* p = nullptr;
    const double* q = nullptr;
    int m = 0, n = 0;
    double bk1 = 0.0, tk = 0.0;
    int M() const { return m + n; }
};

struct HybridOut {
    int itamg = 0;
    double resamg = 0.0;
    long long num_comp = 0, it_num = 0;
};
// Row f3, reuse across Newton steps: the hierarchies of the previous Hybrid_AMG / AMG4POT call of
// a driver, kept alive so that a step whose system is the SAME (same active set, T, bk1, tk: the
// caller says so in `same`) shares their rand-independent levels 1-2 through amg_setup's donor
// mechanism.  Guesses and levels >= 3 still draw the stream's next numbers, so results and the
// count of consumed numbers are those of a full setup, bit for bit.
struct StepDonors {
    std::vector<std::shared_ptr<ipd_amg>> prev;   // in order of use (large components)
    bool same = false;                            // set by the caller before each call
    long long steps = 0, same_steps = 0, shared = 0;   // calls, calls with `same`, donated setups
};

// ---------------------------------------------------------------------------------------------------------------
// ipd_newton_sys.hip: assembly and the vector helpers of the system
// ---------------------------------------------------------------------------------------------------------------
// prob_data of the host ABI on the device, out of ctx->scratch; pot: with z(end), s and phi (AMG4POT, PCG4POT)
struct ProbDev {
    NewtonSys sys;
    const double* z = nullptr;
    const uint8_t* s = nullptr;
    const double* phi = nullptr;
    double* zeta = nullptr;
    size_t len = 0;   // entries of z and zeta: M, or M + 1 with pot
};
ProbDev upload_prob(ipd_ctx* ctx, const ipd_prob* pd, bool pot);
template <class IT>
inline void report(const HybridOut& ho, IT* it, double* res, int64_t info[2]) {
    if (it) *it = ho.itamg;
    if (res) *res = ho.resamg;
    if (info) {
        info[0] = ho.num_comp;
        info[1] = ho.it_num;
    }
}
void build_Ae(ipd_ctx* ctx, Arena& dst, const NewtonSys& sys, Csr* Ae);            // Hybrid_AMG.m:17-24
void scale_qp(ipd_ctx* ctx, const NewtonSys& sys, const double* in, double* out);  // out = Q0*in
void diag_k(ipd_ctx* ctx, const NewtonSys& sys, double* dK);                       // dK = diag(Q0*T*Q0)
// Jk = bk1*I + (T + H0)/tk (APD_SsN_Class1.m:151, inner_solver = 2)
void build_jk(ipd_ctx* ctx, Arena& dst, const NewtonSys& sys, Csr* J);
// Aek = Ae(pk, pk) of one component after another, pk ascending
struct ComponentCutter {
    ipd_ctx* ctx;
    const Csr& Ae;
    std::vector<int> newidx;
    int* d_new;
    ComponentCutter(ipd_ctx* ctx, const Csr& Ae);
    const int* cut(const int* pk, int nk, Csr* Ak);   // returns pk on the device (its own allocation per component)
};
void gather_dev(ipd_ctx* ctx, int nk, const int* pk, const double* src, double* dst);    // dst = src(pk)
void scatter_dev(ipd_ctx* ctx, int nk, const int* pk, const double* src, double* dst);   // dst(pk) = src
double host_sum(ipd_ctx* ctx, const double* d, int n);
double host_dot(ipd_ctx* ctx, const double* a, const double* b, int n);

// ---------------------------------------------------------------------------------------------------------------
// ipd_components.hip
// ---------------------------------------------------------------------------------------------------------------
void find_components(ipd_ctx* ctx, const Csr& A, Components* out);
struct CompOrderScope {   // clears the injected order when the top-level call ends
    ipd_ctx* ctx;
    explicit CompOrderScope(ipd_ctx* c) : ctx(c) {}
    ~CompOrderScope() {
        if (ctx) ctx->comp_order.clear();
    }
};

// ---------------------------------------------------------------------------------------------------------------
// ipd_hybrid.hip
// ---------------------------------------------------------------------------------------------------------------
// Work postponed to the solve phase of a Hybrid_AMG call: AMG4POT's two calls set their
// hierarchies up one after the other (that keeps the order in which the reference consumes
// rand) and then run their solve phases concurrently on two streams.
using Deferred = std::vector<std::function<void()>>;
struct SystemCache {   // Ae and the components, made by the first of AMG4POT's two solves for the second
    bool valid = false;
    Csr Ae;
    Components cc;
};
// What one Hybrid_AMG call shares with others: the rule it was given, and what the rule points at
struct HybridCall {
    explicit HybridCall(const Sharing& r) : rule(r) {}
    const Sharing rule;
    const std::vector<std::shared_ptr<ipd_amg>>* donors = nullptr;   // rule.from's hierarchies, in visiting order
    size_t next_donor = 0;
    std::vector<std::shared_ptr<ipd_amg>> recorded;                  // rule.record: set up by this call
    long long* shared = nullptr;                                     // rule.count: StepDonors::shared
    SystemCache* system = nullptr;                                   // rule.system
};
// later != NULL: the solve phase is appended to it, not run
void hybrid_amg(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const AmgOpts& opts, ipd_rng* rng, double* zeta,
                HybridOut* out, HybridCall& call, Deferred* later);
// opts.twogrid selects Hybrid_twogrid.m (twogrid_bigph on every large component)
void hybrid_amg_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const AmgOpts& opts, ipd_rng* rng,
                    double* zeta, HybridOut* out, StepDonors* step = nullptr);
AmgOpts amg_fill_krylov(const ipd_amg_opts* o);

// ---------------------------------------------------------------------------------------------------------------
// ipd_pot.hip: Class 2's bordered systems
// ---------------------------------------------------------------------------------------------------------------
void amg4pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi,
                 const AmgOpts& opts, ipd_rng* rng, double* zeta, HybridOut* out, StepDonors* step = nullptr);
// Class 2, inner_solver = 1 / 2: direct solve resp. PCG on the bordered Jacobian itself
// (APD_SsN_Class2.m:152-161)
void direct_pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi,
                    double* zeta);
void pcg_pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi, double tol,
                 long long maxit, double* zeta, HybridOut* out);
// PCG4POT (Class2/PCG4POT.m:27-39) = AMG4POT's reduction with aug_PCG as the inner solve
void pcg4pot_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, const uint8_t* s, const double* phi, double tol,
                 long long maxit, double* zeta, HybridOut* out);

// ---------------------------------------------------------------------------------------------------------------
// ipd_aug.hip: aug_PCG.m (inner_solver = 3): PCG on the kernel-augmented system
// ---------------------------------------------------------------------------------------------------------------
void aug_pcg_dev(ipd_ctx* ctx, const NewtonSys& sys, const double* z, double tol, long long maxit, double* zeta,
                 HybridOut* out);
