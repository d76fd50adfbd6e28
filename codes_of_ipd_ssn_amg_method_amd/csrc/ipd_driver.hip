// APD / semismooth-Newton drivers on device-resident vectors:
//   Class1/APD_SsN_Class1.m:101-275, Class2/APD_SsN_Class2.m:95-285.
// This unit holds the workspace, one iteration of the script (apd_iterate), the test whether a
// Newton step meets the previous step's system again, and the C ABI.  The script's scalar decisions
// are ipd_apd_script.h's; the mn-sized passes are ipd_apd_passes.hip's, the warm start is
// ipd_apd_warm.hip's.
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <limits>

#include "ipd_apd_state.h"
#include "ipd_kkt.h"

static_assert(MK == IPD_APD_MERIT_STEPS, "ipd_apd_merit takes MK steps");

namespace {

// Row f3: is this Newton step's system the previous one's?  Compares the active-set mask (and,
// class 2, the 0/1 diagonal of T) with the copies kept from the last step, refreshes the copies
// and raises *changed on any difference.  8-byte words; the caller pads the mask to a multiple.
__global__ void k_words_changed(size_t nw, const unsigned long long* __restrict__ cur,
                                unsigned long long* __restrict__ prev, int* __restrict__ changed) {
    bool diff = false;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < nw;
         i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long c = cur[i];
        if (c != prev[i]) {
            diff = true;
            prev[i] = c;
        }
    }
    if (__any(diff) && (threadIdx.x & 63) == 0) atomicOr(changed, 1);
}

__global__ void k_negate(int n, const double* __restrict__ x, double* __restrict__ y) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        y[i] = -x[i];
}

void push_hist(ipd_apd* h) {
    h->h_fx.push_back(h->fval);
    h->h_kx.push_back(h->kkt[0]);
    h->h_kl.push_back(h->kkt[1]);
    h->h_ky.push_back(h->kkt[2]);
    h->h_kz.push_back(h->kkt[3]);
}

void ensure_kkt(ipd_apd* h) {
    if (h->have_kkt) return;
    apd_end(h, false, h->u, h->lam, h->kkt, &h->fval);   // Class1 :63-65, Class2 :44-48
    for (int i = 0; i < 4; ++i) h->kkt0[i] = h->kkt[i];
    h->h_fx.clear();
    h->h_kx.clear();
    h->h_kl.clear();
    h->h_ky.clear();
    h->h_kz.clear();
    h->h_ssn.clear();
    push_hist(h);
    h->have_kkt = true;
}

// Row f3: true when the system of this Newton step (active set, class 2's T, bk1, tk; p and q
// never change) is the one the previous step's hierarchies were built for.
bool step_same_system(ipd_apd* h, double bk1, double tk) {
    ipd_ctx* ctx = h->ctx;
    IPD_HIP(hipMemsetAsync(h->step_changed, 0, sizeof(int), ctx->stream));
    hipLaunchKernelGGL(k_words_changed, dim3(std::max(1, std::min(cdiv((int)std::min<size_t>(h->s_words, 1u << 30), 256), 1024))),
                       dim3(256), 0, ctx->stream, h->s_words,
                       reinterpret_cast<const unsigned long long*>(h->s), h->s_prev, h->step_changed);
    if (h->tmask)
        hipLaunchKernelGGL(k_words_changed, dim3(cdiv(h->M, 256)), dim3(256), 0, ctx->stream,
                           (size_t)h->M, reinterpret_cast<const unsigned long long*>(h->tmask),
                           h->t_prev, h->step_changed);
    IPD_KERNEL_CHECK();
    const bool changed = ctx->fetch1(h->step_changed) != 0;
    const bool same = h->have_prev && !changed && bk1 == h->prev_bk1 && tk == h->prev_tk;
    h->have_prev = true;
    h->prev_bk1 = bk1;
    h->prev_tk = tk;
    return same;
}

// zeta = Jk \ (-Fk_old), -Fk_old in h->negF, by the route of (class, inner_solver)
//                                                          :146-161 / Class2 :152-171
void newton_direction(ipd_apd* h, const ipd_apd_opts& o, const AmgOpts& amg, ipd_rng* rng, const Csr& H0,
                      StepDonors* step, HybridOut* ho) {
    ipd_ctx* ctx = h->ctx;
    const double* z = h->negF;
    NewtonSys sys;
    sys.H0 = H0;
    sys.tdiag = h->cls == 2 ? h->tmask : nullptr;
    sys.p = h->p;
    sys.q = h->q;
    sys.m = h->m;
    sys.n = h->n;
    sys.bk1 = h->bk1;
    sys.tk = h->tk;
    switch (apd_route(h->cls == 2, o.inner_solver)) {
        case ROUTE_DIRECT: {                                       // :146-148
            Csr Jk;
            build_jk(ctx, *ctx->scratch, sys, &Jk);
            spd_solve_dev(ctx, Jk, z, h->zeta);
            ho->itamg = 1;                                         // itpcg = 1; respcg = 0; info = [0,0]
            ho->resamg = 0.0;
            break;
        }
        case ROUTE_DIRECT_POT:                                     // Class2 :152-156
            direct_pot_dev(ctx, sys, z, h->s, h->phi, h->zeta);
            ho->itamg = 1;
            ho->resamg = 0.0;
            break;
        case ROUTE_PCG: {                                          // :149-152  PCG(Jk,-Fk_old)
            Csr Jk;
            build_jk(ctx, *ctx->scratch, sys, &Jk);
            long long it2 = 0;
            double res2 = 0.0;
            pcg_dev(ctx, Jk, z, nullptr, o.pcg_retol, o.pcg_maxit, 2, h->zeta, &it2, &res2, nullptr);
            ho->itamg = (int)std::min<long long>(it2, 2147483647LL);
            ho->resamg = res2;
            break;
        }
        case ROUTE_PCG_POT:                                        // Class2 :157-161  PCG on the bordered Jk
            pcg_pot_dev(ctx, sys, z, h->s, h->phi, o.pcg_retol, o.pcg_maxit, h->zeta, ho);
            break;
        case ROUTE_AUG_PCG:                                        // :157-159
            aug_pcg_dev(ctx, sys, z, o.pcg_retol, o.pcg_maxit, h->zeta, ho);
            break;
        case ROUTE_PCG4POT:                                        // Class2 :167-169
            pcg4pot_dev(ctx, sys, z, h->s, h->phi, o.pcg_retol, o.pcg_maxit, h->zeta, ho);
            break;
        case ROUTE_HYBRID_AMG:                                     // Class1 :161
            hybrid_amg_dev(ctx, sys, z, amg, rng, h->zeta, ho, step);
            break;
        case ROUTE_AMG4POT:                                        // Class2 :171
            amg4pot_dev(ctx, sys, z, h->s, h->phi, amg, rng, h->zeta, ho, step);
            break;
    }
}

// one APD iteration                                       Class1 :101-275, Class2 :95-285
void apd_iterate(ipd_apd* h, const ipd_apd_opts& o, const AmgOpts& amg, ipd_rng* rng) {
    const int solver = o.inner_solver;
    ipd_ctx* ctx = h->ctx;
    const int k = ++h->k;
    const bool c2 = h->cls == 2;
    const double resk = apd_resk(c2, h->kkt);
    apd_begin(h, k);
    const double bk1 = h->bk1, tk = h->tk;
    const double ssn_tol = apd_ssn_tol(k, bk1, o.ssn_tol1);                       // :123
    const bool merit3 = !c2 && o.prob >= 3;
    h->merit3 = merit3;
    auto merit = [&](const EvalRes& e) {                                          // :182
        return apd_merit_value(merit3, bk1, tk, e.lam2, e.wlk_lam, e.prox2, e.z2, e.zmp2);
    };
    // :128-131  lk_new = lk ; Fk_new
    double* lam_new = h->lam_a;
    double* lam_old = h->lam_b;
    double* F_new = h->F_a;
    double* F_old = h->F_b;
    EvalRes e_new = apd_eval(h, merit3, h->lam, nullptr, 0.0, lam_new, F_new, nullptr);
    int ssn_it = 0;
    long long psum = 0;
    while (apd_ssn_wants_step(e_new.normF, ssn_tol)) {                            // :137
        ++ssn_it;
        std::swap(lam_new, lam_old);
        std::swap(F_new, F_old);
        const EvalRes e_old = e_new;   // same multiplier, same pass: s, Fk_old, cFk_old (:139-144)
        Csr H0;
        HybridOut ho;
        {
            CallScope scope(ctx);
            {
                ProfScope ps(ctx, PROF_ASAT);
                kkt_asat(ctx, *ctx->scratch, h->s, h->p, h->q, h->m, h->n, &H0);   // :142
            }
            hipLaunchKernelGGL(k_negate, dim3(cdiv(h->L, 256)), dim3(256), 0, ctx->stream, h->L,
                               (const double*)F_old, h->negF);                     // z = -Fk_old
            IPD_KERNEL_CHECK();
            StepDonors* donors = nullptr;
            if (h->step_reuse && solver == 4) {
                donors = &h->step;
                donors->same = step_same_system(h, bk1, tk);
                ++donors->steps;
                donors->same_steps += donors->same;
            } else {
                h->have_prev = false;
                h->step.prev.clear();
            }
            newton_direction(h, o, amg, rng, H0, donors, &ho);
        }
        const int itpcg = ho.itamg;
        if (solver >= 4) {
            if (itpcg == amg.maxit)
                ++h->fail_amg;                                                     // :163-169
            else
                h->max_amg = std::max<long long>(h->max_amg, itpcg);
            if (itpcg > 0) ++h->total_amg;
        }
        psum += itpcg;
        // :182-211 line search
        const double cF_old = merit(e_old);
        int ll = 0;
        double step = 1.0;
        e_new = apd_eval(h, merit3, lam_old, h->zeta, step, lam_new, F_new, F_old);
        const double ress = std::fabs(e_new.fold_zeta);                            // :198
        if (apd_ls_batched(apd_armijo_rejects(merit(e_new), cF_old, o.nu, step, ress), merit3, o.ll_max)) {
            // the trials that follow only decide on the merit: MK of them per pass over wk,
            // then one full evaluation at the accepted (or last) step
            bool found = false;
            while (!found && ll < o.ll_max) {
                double st[MK], mv[MK];
                apd_batch_steps(o.delta, ll, st);
                apd_merit(h, lam_old, h->zeta, st, mv);
                found = apd_batch_pick(mv, st, cF_old, o.nu, ress, o.ll_max, &ll);
            }
            ll = apd_ls_clamp(ll, o.ll_max);
            step = apd_trial_step(o.delta, ll);
            e_new = apd_eval(h, merit3, lam_old, h->zeta, step, lam_new, F_new, F_old);
        } else {
            while (apd_armijo_rejects(merit(e_new), cF_old, o.nu, step, ress)) {   // :199
                ++ll;
                step = apd_trial_step(o.delta, ll);
                e_new = apd_eval(h, merit3, lam_old, h->zeta, step, lam_new, F_new, F_old);
                if (ll == o.ll_max) break;
            }
        }
        ipd_ssn_rec rec;
        rec.k = k;
        rec.ssn_it = ssn_it;
        rec.ll = ll;
        rec.itamg = itpcg;
        rec.E = e_old.E;
        rec.info0 = ho.num_comp;
        rec.info1 = ho.it_num;
        rec.Fk_norm = e_new.normF;
        rec.resamg = ho.resamg;
        rec.bk1 = bk1;
        rec.tk = tk;
        h->recs.push_back(rec);
        if (apd_ssn_solved(e_new.normF, ssn_tol)) break;                           // :213
        if (apd_ssn_stalled(c2, e_old.normF, e_new.normF, ssn_tol)) break;         // :219 / Class2 :207
        if (apd_ssn_exhausted(ssn_it, o.ssn_it)) break;                            // :226
    }
    // :239-254
    double kk[4], fx;
    apd_end(h, true, nullptr, lam_new, kk, &fx);
    double rr = apd_max_rr(c2, kk, h->kkt0);
    double bk_next = bk1;
    if (apd_restarts(bk1, rr, resk)) {                                             // :245
        copy_dev(h, h->v, h->u, h->U);                                             // vk1 = xk
        if (c2) {
            bk_next = apd_restart_bk_class2(bk1);                                  // Class2 :255
        } else {
            // rand (:246) through the stream's fill(): a replayed stream, its exhaustion error and
            // the count of consumed numbers are honoured (next_double() bypassed all three)
            double v = 0.0;
            rng->fill(&v, 1);
            bk_next = v;
        }
        ++h->restarts;
        apd_end(h, false, h->u, h->lam, kk, &fx);
        rr = apd_max_rr(c2, kk, h->kkt0);
    } else {
        std::swap(h->u, h->u2);
        copy_dev(h, h->lam, lam_new, (size_t)h->L);
    }
    h->bk = bk_next;
    for (int i = 0; i < 4; ++i) h->kkt[i] = kk[i];
    h->fval = fx;
    push_hist(h);
    h->h_ssn.push_back((double)ssn_it);
    h->sum_amg += psum;
    if (rr <= o.kkt_tol) h->converged = true;                                      // :266
}

// one probe of the certified gap on the state iteration h->k left: the bracket, the best lower
// bound so far with its multiplier, the record, and at a stop the install the rule asks for.  Every decision is
// ipd_apd_script.h's.
void gap_probe(ipd_apd* h) {
    ipd_ctx* ctx = h->ctx;
    const ipd_gap_rule& rule = h->gap_rule;
    CallScope scope(ctx);
    const BracketRun r = apd_bracket_measure(h, rule.tol);
    ipd_gap_rec rec;
    rec.k = h->k;
    rec.lower_side = r.b.lower_side;
    rec.upper_side = r.b.upper_side;
    rec.upper_ok = r.b.upper.ok;
    rec.final = h->converged ? 1 : 0;
    rec.lower = r.b.lower.dual;
    rec.lower_dmin = r.b.lower.dmin;
    if (apd_gap_improves(rec.lower, h->gap_best)) {
        copy_dev(h, h->gap_lam, r.lam[r.b.lower_side], (size_t)h->L);
        h->gap_have_lam = true;
    }
    h->gap_best = apd_gap_best(rec.lower, h->gap_best);
    rec.best = h->gap_best;
    rec.upper = r.b.upper.fval;
    rec.viol_in = r.b.upper.viol_in;
    rec.gap = apd_gap_value(rec.upper, rec.best);
    const double thr = apd_gap_threshold(rule.gap_tol, rule.gap_rel, rec.upper);
    rec.stop = apd_gap_stops(thr, rec.upper_ok, rec.gap) ? 1 : 0;
    if (rec.stop) {
        h->gap_stopped = true;
        if (rule.install) apd_bracket_install(h, r);
    }
    ctx->sync();   // the scratch arrays are the next call's
    h->gap_recs.push_back(rec);
}

void fill_result(const ipd_apd* h, ipd_apd_result* r) {
    r->converged = h->converged ? 1 : 0;
    r->k = h->k;
    r->fval = h->fval;
    r->kkt[0] = h->kkt[0];
    r->kkt[1] = h->kkt[1];
    r->kkt[2] = h->kkt[2];
    r->kkt[3] = h->kkt[3];
    r->rr = h->have_kkt ? apd_max_rr(h->cls == 2, h->kkt, h->kkt0) : 0.0;
    r->sum_amg = h->sum_amg;
    r->total_amg = h->total_amg;
    r->fail_amg = h->fail_amg;
    r->max_amg = h->max_amg;
    r->restarts = h->restarts;
    r->nrec = (int64_t)h->recs.size();
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" void ipd_apd_opts_init(int32_t cls, ipd_apd_opts* o) {
    if (!o) return;
    o->maxit = 100;
    o->kkt_tol = 1e-6;
    o->ssn_it = 50;
    o->ssn_tol1 = cls == 2 ? 1e-10 : 1e-11;
    o->nu = 0.2;
    o->delta = 0.9;
    o->ll_max = 500;
    o->prob = 2;
    o->inner_solver = 4;
    o->pcg_retol = 1e-11;
    o->pcg_maxit = 10000;
}

// The one body of ipd_apd_create, ipd_apd_create_points and ipd_apd_create_points_free (ipd_cost.hip): without
// fill and free_fill c (and phi) come from the host arrays of *d, fill makes them on the device, and free_fill
// keeps the coordinates in place of c.
void apd_create_common(ipd_ctx* ctx, const ipd_apd_data* d, const ApdCostFill* fill, ipd_apd** out,
                       const ApdCostFree* free_fill) {
    IPD_REQUIRE(ctx && d && out, IPD_E_ARG, "NULL argument");
    IPD_REQUIRE(d->cls == 1 || d->cls == 2, IPD_E_ARG, "cls must be 1 or 2");
    IPD_REQUIRE(d->m > 0 && d->n > 0 && d->m <= IPD_APD_SIDE_MAX && d->n <= IPD_APD_SIDE_MAX, IPD_E_LIMIT,
                "m, n must be in [1, 16384]");
    IPD_REQUIRE((fill || free_fill || d->c) && d->r && d->l && d->p && d->q, IPD_E_ARG, "NULL problem vector");
    IPD_REQUIRE(d->cls == 1 || d->phi || fill || free_fill, IPD_E_ARG, "class 2 needs phi");
    ctx->set_device();
    std::unique_ptr<ipd_apd> h(new ipd_apd);
    h->ctx = ctx;
    h->arena.reset(new Arena(&ctx->pool));
    Arena& A = *h->arena;
    const int m = (int)d->m, n = (int)d->n;
    h->cls = d->cls;
    h->m = m;
    h->n = n;
    h->M = m + n;
    h->L = h->M + (d->cls == 2 ? 1 : 0);
    h->mn = (size_t)m * n;
    h->U = h->mn + (d->cls == 2 ? (size_t)h->M : 0);
    h->mu = d->mu;
    const int forced_reps = apd_reps_switch(switch_value("IPD_APD_REPS"));
    IPD_REQUIRE(forced_reps >= 0, IPD_E_ARG, "IPD_APD_REPS must be 1, 2, 4 or 8");
    h->geo = make_geo(m, n, forced_reps);
    const size_t mn = h->mn, U = h->U;
    const int L = h->L;
    if (!free_fill) h->c = A.alloc<double>(mn);   // matrix-free: c stays nullptr
    h->p = A.alloc<double>((size_t)m);
    h->q = A.alloc<double>((size_t)n);
    h->b = A.alloc<double>((size_t)L);
    if (!fill && !free_fill) ctx->upload(h->c, d->c, mn);
    ctx->upload(h->p, d->p, (size_t)m);
    ctx->upload(h->q, d->q, (size_t)n);
    ctx->upload(h->b, d->r, (size_t)n);            // b = [r;l(;mu)]  (:33 / Class2 :29)
    ctx->upload(h->b + n, d->l, (size_t)m);
    if (d->cls == 2) {
        ctx->upload(h->b + h->M, &d->mu, 1);
        h->phi = A.alloc<double>(mn);
        if (d->phi) ctx->upload(h->phi, d->phi, mn);
        h->tmask = A.alloc<double>((size_t)h->M);
        h->phi_l = A.alloc<double>((size_t)h->M);
        h->phi_part = A.alloc<double>(PHI_PARTS_MAX);
    } else if (d->gama) {
        h->gama = A.alloc<double>(mn);
        ctx->upload(h->gama, d->gama, mn);
    }
    h->u = A.alloc<double>(U);
    h->u2 = A.alloc<double>(U);
    h->v = A.alloc<double>(U);
    h->w = A.alloc<double>(U);
    for (double* a : {h->u, h->u2, h->v, h->w})
        IPD_HIP(hipMemsetAsync(a, 0, U * sizeof(double), ctx->stream));
    h->lam = A.alloc<double>((size_t)L);
    h->lam_a = A.alloc<double>((size_t)L);
    h->lam_b = A.alloc<double>((size_t)L);
    h->wlk = A.alloc<double>((size_t)L);
    h->F_a = A.alloc<double>((size_t)L);
    h->F_b = A.alloc<double>((size_t)L);
    h->zeta = A.alloc<double>((size_t)L);
    h->negF = A.alloc<double>((size_t)L);
    for (double* a : {h->lam, h->lam_a, h->lam_b, h->wlk, h->F_a, h->F_b, h->zeta, h->negF})
        IPD_HIP(hipMemsetAsync(a, 0, (size_t)L * sizeof(double), ctx->stream));
    h->s_words = (mn + 7) / 8;                      // compared in 8-byte words (row f3)
    h->s = A.alloc<uint8_t>(h->s_words * 8);
    IPD_HIP(hipMemsetAsync(h->s, 0, h->s_words * 8, ctx->stream));
    h->s_prev = A.alloc<unsigned long long>(h->s_words);
    if (d->cls == 2) h->t_prev = A.alloc<unsigned long long>((size_t)h->M);
    h->step_changed = A.alloc<int>(1);
    h->step_reuse = !switch_on("IPD_NO_STEP_DONOR");
    const Geo& g = h->geo;
    h->lpart = A.alloc<double>(apd_lpart_len(g));
    h->rpart = A.alloc<double>(apd_rpart_len(g));
    IPD_HIP(hipMemsetAsync(h->rpart, 0, sizeof(double) * apd_rpart_len(g), ctx->stream));
    h->spart = A.alloc<double>(apd_nblk(g) * NSC);
    h->dscal = reinterpret_cast<ApdScal*>(A.alloc<double>(sizeof(ApdScal) / sizeof(double) + 1));
    h->fpart = A.alloc<double>(apd_fpart_len(L));
    h->merit = A.alloc<double>(MK);
    h->counter = A.alloc<int>(4);
    IPD_HIP(hipMemsetAsync(h->counter, 0, 16, ctx->stream));
    Prob& P = h->P;
    P.cls2 = d->cls == 2 ? 1 : 0;
    P.m = m;
    P.n = n;
    P.p = h->p;
    P.q = h->q;
    P.c = h->c;
    P.phi = h->phi;
    P.gama = h->gama;
    P.gs = d->cls == 2 ? std::numeric_limits<double>::infinity() : d->gama_scalar;
    if (fill) {
        (*fill)(h->c, d->cls == 2 && !d->phi ? h->phi : nullptr, &h->cost_stats);
        h->have_cost_stats = true;
    } else if (free_fill) {
        (*free_fill)(h.get(), d->cls == 2 && !d->phi ? h->phi : nullptr);
        h->have_cost_stats = true;
    }
    if (d->cls == 2) {
        CallScope scope(ctx);
        h->phi_npart = kkt_phi_consts(ctx, h->phi, h->p, h->q, m, n, h->phi_l, h->phi_part);
    }
    ctx->sync();
    *out = h.release();
}

extern "C" int ipd_apd_create(ipd_ctx* ctx, const ipd_apd_data* d, ipd_apd** out) {
    return ipd_guard([&] { apd_create_common(ctx, d, nullptr, out); });
}

extern "C" void ipd_apd_destroy(ipd_apd* h) {
    if (!h) return;
    try {
        h->ctx->set_device();
        h->ctx->sync();
    } catch (...) {
    }
    delete h;
}

extern "C" int ipd_apd_dims(const ipd_apd* h, int64_t* len_u, int64_t* len_lam) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        if (len_u) *len_u = (int64_t)h->U;
        if (len_lam) *len_lam = (int64_t)h->L;
    });
}

extern "C" int ipd_apd_warmup(ipd_apd* h, double res, int64_t maxit) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        const bool inf = maxit < 0;
        IPD_REQUIRE(!(res == 0.0 && inf), IPD_E_ARG, "res = 0 and maxit = inf");   // :10-12
        long long its = inf ? 500 : (long long)maxit;                                // :18-20
        apd_warmup(h, res, its);
    });
}

extern "C" int ipd_apd_set_state(ipd_apd* h, const double* u, const double* v, const double* lam,
                                 double bk) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        IPD_REQUIRE(bk > 0.0, IPD_E_ARG, "bk must be positive");
        h->ctx->set_device();
        if (u) h->ctx->upload(h->u, u, h->U);
        if (v) h->ctx->upload(h->v, v, h->U);
        if (lam) h->ctx->upload(h->lam, lam, (size_t)h->L);
        h->bk = bk;
        apd_restart_script(h);
    });
}

void apd_restart_script(ipd_apd* h) {
    h->k = 0;
    h->have_kkt = false;
    h->converged = false;
    h->recs.clear();
    h->sum_amg = h->total_amg = h->fail_amg = h->max_amg = 0;
    h->restarts = 0;
    h->gap_stopped = false;
    h->gap_have_lam = false;
    h->gap_best = -std::numeric_limits<double>::infinity();
    h->gap_recs.clear();
}

extern "C" int ipd_apd_set_krylov(ipd_apd* h, int32_t on) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        h->krylov = on != 0;
    });
}

extern "C" int ipd_apd_get_state(ipd_apd* h, double* u, double* v, double* lam, double* bk) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        h->ctx->set_device();
        if (u) h->ctx->fetch(h->u, u, h->U);
        if (v) h->ctx->fetch(h->v, v, h->U);
        if (lam) h->ctx->fetch(h->lam, lam, (size_t)h->L);
        if (bk) *bk = h->bk;
    });
}

extern "C" int ipd_apd_run(ipd_apd* h, const ipd_apd_opts* o, const ipd_amg_opts* amg,
                           ipd_rng* rng, int32_t iters, ipd_apd_result* res) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && rng, IPD_E_ARG, "NULL argument");
        h->ctx->comp_order.clear();   // a recorded component order belongs to ONE Newton system
        ipd_apd_opts oo;
        if (o)
            oo = *o;
        else
            ipd_apd_opts_init(h->cls, &oo);
        IPD_REQUIRE(oo.maxit > 0 && oo.ssn_it > 0 && oo.ll_max >= 0 && oo.delta > 0.0 &&
                        oo.delta < 1.0,
                    IPD_E_ARG, "bad driver options");
        IPD_REQUIRE(oo.inner_solver >= 1 && oo.inner_solver <= 5, IPD_E_ARG,
                    "inner_solver must be 1 (direct), 2 (PCG), 3 (aug_PCG / PCG4POT), 4 (AMG) or 5 (two-grid)");
        AmgOpts ao = oo.inner_solver == 5 ? amg_fill_twogrid_defaults(amg) : amg_fill_defaults(amg);
        ao.krylov = h->krylov && oo.inner_solver == 4;
        h->ctx->set_device();
        ensure_kkt(h);
        for (int it = 0; it < iters && h->k < oo.maxit && !h->converged && !h->gap_stopped; ++it) {
            apd_iterate(h, oo, ao, rng);
            if (h->gap_on && apd_gap_due(h->k, h->gap_rule.first, h->gap_rule.every, h->converged)) gap_probe(h);
        }
        h->ctx->sync();
        if (res) fill_result(h, res);
    });
}

extern "C" int ipd_apd_set_gap_rule(ipd_apd* h, const ipd_gap_rule* r) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        if (!r) {
            h->gap_on = false;
            h->gap_stopped = false;
            return;
        }
        IPD_REQUIRE(!apd_dual_cap_on(h), IPD_E_UNSUPPORTED,
                    "ipd_apd_set_gap_rule: the bracket does not apply with finite gama");
        IPD_REQUIRE(r->gap_tol >= 0.0 && r->gap_rel >= 0.0 && r->tol >= 0.0, IPD_E_ARG,   // a NaN fails the comparison
                    "ipd_apd_set_gap_rule: gap_tol, gap_rel and tol must be >= 0");
        IPD_REQUIRE(std::isfinite(r->gap_tol) && std::isfinite(r->gap_rel), IPD_E_ARG,
                    "ipd_apd_set_gap_rule: gap_tol and gap_rel must be finite");
        IPD_REQUIRE(r->first >= 1 && r->every >= 1, IPD_E_ARG, "ipd_apd_set_gap_rule: first and every must be >= 1");
        IPD_REQUIRE(r->install == 0 || r->install == 1, IPD_E_ARG, "ipd_apd_set_gap_rule: install must be 0 or 1");
        h->ctx->set_device();
        apd_dual_check_divider(h, 0);
        apd_dual_check_divider(h, 1);
        if (!h->gap_lam) h->gap_lam = h->arena->alloc<double>((size_t)h->L);
        h->gap_rule = *r;
        h->gap_on = true;
        h->gap_stopped = false;
    });
}

extern "C" int ipd_apd_gap_records(const ipd_apd* h, ipd_gap_rec* out, int64_t cap, int64_t* count) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && count, IPD_E_ARG, "NULL argument");
        const int64_t nn = std::min<int64_t>(cap, (int64_t)h->gap_recs.size());
        if (out)
            for (int64_t i = 0; i < nn; ++i) out[i] = h->gap_recs[(size_t)i];
        *count = (int64_t)h->gap_recs.size();
    });
}

extern "C" int ipd_apd_gap_lam(ipd_apd* h, double* lam, double* best) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        if (lam && h->gap_have_lam) {
            h->ctx->set_device();
            h->ctx->fetch(h->gap_lam, lam, (size_t)h->L);
        }
        if (best) *best = h->gap_best;
    });
}

extern "C" int ipd_apd_history(const ipd_apd* h, int32_t which, double* out, int64_t cap,
                               int64_t* count) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && count, IPD_E_ARG, "NULL argument");
        const std::vector<double>* src = nullptr;
        switch (which) {
            case 0: src = &h->h_fx; break;
            case 1: src = &h->h_kx; break;
            case 2: src = &h->h_kl; break;
            case 3: src = &h->h_ky; break;
            case 4: src = &h->h_kz; break;
            case 5: src = &h->h_ssn; break;
            default: throw IpdError(IPD_E_ARG, "history selector must be 0..5");
        }
        const int64_t nn = std::min<int64_t>(cap, (int64_t)src->size());
        if (out)
            for (int64_t i = 0; i < nn; ++i) out[i] = (*src)[(size_t)i];
        *count = (int64_t)src->size();
    });
}

extern "C" int ipd_apd_reuse_stats(const ipd_apd* h, int64_t* steps, int64_t* same_system,
                                   int64_t* donated) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        if (steps) *steps = h->step.steps;
        if (same_system) *same_system = h->step.same_steps;
        if (donated) *donated = h->step.shared;
    });
}

extern "C" int ipd_apd_records(const ipd_apd* h, ipd_ssn_rec* out, int64_t cap, int64_t* count) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && count, IPD_E_ARG, "NULL argument");
        const int64_t nn = std::min<int64_t>(cap, (int64_t)h->recs.size());
        if (out)
            for (int64_t i = 0; i < nn; ++i) out[i] = h->recs[(size_t)i];
        *count = (int64_t)h->recs.size();
    });
}

extern "C" int ipd_apd_begin(ipd_apd* h, int32_t k, double vals[3]) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && k >= 1, IPD_E_ARG, "bad argument");
        h->ctx->set_device();
        apd_begin(h, k);
        h->ctx->sync();
        if (vals) {
            vals[0] = h->bk1;
            vals[1] = h->tk;
            vals[2] = h->ak;
        }
    });
}

extern "C" int ipd_apd_eval(ipd_apd* h, const double* lam, uint8_t* s_out, double* t_out,
                            double* Fk_out, double vals[6]) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && lam, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(h->tk > 0.0, IPD_E_ARG, "ipd_apd_begin must run first");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        ctx->upload(h->lam_a, lam, (size_t)h->L);
        const EvalRes e = apd_eval(h, h->merit3, h->lam_a, nullptr, 0.0, nullptr, h->F_a, nullptr);
        if (s_out) ctx->fetch(h->s, s_out, h->mn);
        if (t_out && h->tmask) ctx->fetch(h->tmask, t_out, (size_t)h->M);
        if (Fk_out) ctx->fetch(h->F_a, Fk_out, (size_t)h->L);
        if (vals) {
            vals[0] = h->bk1;
            vals[1] = h->tk;
            vals[2] = h->ak;
            vals[3] = e.normF;
            vals[4] = apd_merit_value(false, h->bk1, h->tk, e.lam2, e.wlk_lam, e.prox2, e.z2, e.zmp2);   // the prob < 3 form
            vals[5] = (double)e.E;
        }
    });
}

extern "C" int ipd_apd_get_w(ipd_apd* h, double* wk, double* wlk) {
    return ipd_guard([&] {
        IPD_REQUIRE(h, IPD_E_ARG, "NULL handle");
        IPD_REQUIRE(h->tk > 0.0, IPD_E_ARG, "ipd_apd_begin must run first");
        h->ctx->set_device();
        if (wk) h->ctx->fetch(h->w, wk, h->U);
        if (wlk) h->ctx->fetch(h->wlk, wlk, (size_t)h->L);
    });
}

extern "C" int ipd_apd_eval_trial(ipd_apd* h, const double* lam, const double* zeta, double step,
                                  const double* Fk_old, int32_t merit3, uint8_t* s_out, double* t_out,
                                  double* Fk_out, double* lam_out, double vals[12]) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && lam, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(h->tk > 0.0, IPD_E_ARG, "ipd_apd_begin must run first");
        IPD_REQUIRE(!(merit3 && h->cls == 2), IPD_E_ARG, "the prob-3 merit belongs to class 1");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        // the buffers of apd_iterate's line search: lk_old, zeta, Fk_old in; lk_new, Fk_new out
        ctx->upload(h->lam_b, lam, (size_t)h->L);
        if (zeta) ctx->upload(h->zeta, zeta, (size_t)h->L);
        if (zeta && Fk_old) ctx->upload(h->F_b, Fk_old, (size_t)h->L);
        const EvalRes e = apd_eval(h, merit3 != 0, h->lam_b, zeta ? h->zeta : nullptr, step, h->lam_a, h->F_a,
                                   zeta && Fk_old ? h->F_b : nullptr);
        if (s_out) ctx->fetch(h->s, s_out, h->mn);
        if (t_out && h->tmask) ctx->fetch(h->tmask, t_out, (size_t)h->M);
        if (Fk_out) ctx->fetch(h->F_a, Fk_out, (size_t)h->L);
        if (lam_out) ctx->fetch(h->lam_a, lam_out, (size_t)h->L);
        if (vals) {
            vals[0] = h->bk1;
            vals[1] = h->tk;
            vals[2] = h->ak;
            vals[3] = e.normF;
            vals[4] = apd_merit_value(merit3 != 0, h->bk1, h->tk, e.lam2, e.wlk_lam, e.prox2, e.z2, e.zmp2);
            vals[5] = (double)e.E;
            vals[6] = e.z2;
            vals[7] = e.zmp2;
            vals[8] = e.fold_zeta;
            vals[9] = e.lam2;
            vals[10] = e.wlk_lam;
            vals[11] = e.prox2;
        }
    });
}

extern "C" int ipd_apd_merit(ipd_apd* h, const double* lam, const double* zeta,
                             const double steps[IPD_APD_MERIT_STEPS], double merit[IPD_APD_MERIT_STEPS]) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && lam && zeta && steps && merit, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(h->tk > 0.0, IPD_E_ARG, "ipd_apd_begin must run first");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        ctx->upload(h->lam_b, lam, (size_t)h->L);
        ctx->upload(h->zeta, zeta, (size_t)h->L);
        apd_merit(h, h->lam_b, h->zeta, steps, merit);
    });
}

extern "C" int ipd_apd_end(ipd_apd* h, int32_t from_w, const double* lam, const double* u, double kkt[4],
                           double* fx) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && lam && kkt && fx, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(!from_w || h->tk > 0.0, IPD_E_ARG, "ipd_apd_begin must run first");
        IPD_REQUIRE(!(from_w && u), IPD_E_ARG, "from_w measures the iterate it forms: u must be NULL");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        ctx->upload(h->lam_a, lam, (size_t)h->L);
        if (from_w) {
            apd_end(h, true, nullptr, h->lam_a, kkt, fx);
            std::swap(h->u, h->u2);                                            // as apd_iterate without a restart
            copy_dev(h, h->lam, h->lam_a, (size_t)h->L);
        } else {
            if (u) ctx->upload(h->u2, u, h->U);                                // u2 is free between iterations
            apd_end(h, false, u ? h->u2 : h->u, h->lam_a, kkt, fx);
        }
        ctx->sync();
    });
}

extern "C" int ipd_apd_bench_eval(ipd_apd* h, int32_t reps, double* total_ms,
                                  double* bytes_per_pass) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && reps > 0 && total_ms, IPD_E_ARG, "bad argument");
        IPD_REQUIRE(h->tk > 0.0, IPD_E_ARG, "ipd_apd_begin must run first");
        ipd_ctx* ctx = h->ctx;
        ctx->set_device();
        *total_ms = apd_bench_eval(h, h->merit3, reps);
        if (bytes_per_pass) *bytes_per_pass = apd_eval_bytes(h->geo, h->phi != nullptr, h->gama != nullptr);
    });
}
