// AMG setup on the device: one level's transfer (plan, C/F split, interpolation, Galerkin product) and the
// hierarchy loop (AMG/transfer.m:17-66, AMG/Class_AMG.m:41-85).  The coarsening is ipd_coarsen.hip's, the
// interpolation builds are ipd_prolong.hip's, the products ipd_sparse.hip's, and every choice between their forms
// is made in ipd_setup_plan.h.  All of it is integer/compare work or strictly ordered fp64 arithmetic, so C/F
// masks, Pro and Ac are BIT-IDENTICAL to the oracle's on every level.
#pragma clang fp contract(off)

#include "ipd_setup_internal.h"

#include <cmath>

void amg_transfer(ipd_ctx* ctx, Arena& dst, const Csr& A, const AmgOpts& o, int level,
                  ipd_rng* rng, Csr* Ac, Csr* Pout, Csr* Ptout, uint8_t* cmask, Csr* T1out) {
    IPD_REQUIRE(A.nr == A.nc, IPD_E_ARG, "transfer: A must be square");
    IPD_REQUIRE(&dst != ctx->scratch.get(), IPD_E_ARG, "transfer: dst must not be the scratch arena");
    CallScope scope(ctx);  // temporaries die with this call; results live in dst
    Arena& tmp = *ctx->scratch;
    const int N = A.nr;
    const SetupSwitches sw = read_setup_switches();
    int* const hint = transfer_has_hints(level) ? ctx->xfer_hint[level] : nullptr;
    TransferShape shape;
    shape.level = level, shape.N = N, shape.nnz = A.nnz;
    shape.bigph = o.bigph, shape.inter = o.inter, shape.fnode = o.fnode;
    if (hint) std::copy(hint, hint + 4, shape.hint);
    TransferPlan plan;
    Csr P;
    int* counts = nullptr;   // device, lazy counts: entries of P, P'A, Ac; a flag (bigraph level: Aff not diagonal); longest row of P'A
    if (transfer_is_bigraph(shape)) {                                        // transfer.m:19-25
        const int nf = (int)o.fnode;
        IPD_REQUIRE(nf > 0 && nf < N, IPD_E_ARG, "transfer: fnode must satisfy 0 < fnode < N");
        plan = plan_transfer(shape, N - nf, sw);
        if (plan.lazy) counts = zeroed<int>(ctx, 6);
        amg_prolong_bigraph(ctx, dst, A, o, plan, counts, cmask, &P);
    } else {                                                                 // transfer.m:41-63
        LevelSplit s;
        s.isC = cmask;
        s.isF = tmp.alloc<uint8_t>((size_t)N);
        s.strong = tmp.alloc<uint8_t>((size_t)std::max(A.nnz, 1));
        s.cidx = tmp.alloc<int>((size_t)N + 2);  // cidx[N] = Nc, cidx[N+1] = #bad
        s.maxrow = tmp.alloc<double>((size_t)N);
        s.diag = tmp.alloc<double>((size_t)N);
        amg_level_split(ctx, A, o.theta, rng, plan_mis_small(N, A.nnz, sw), &s);
        IPD_REQUIRE(s.bad == 0, IPD_E_NUMERIC,
                    "mis_set left nodes in neither/both of the C and F sets (SURVEY A-6)");
        IPD_REQUIRE(s.Nc > 0, IPD_E_NUMERIC, "transfer: empty coarse set");
        IPD_REQUIRE(s.Nc <= XFER_COARSE_MAX, IPD_E_LIMIT,
                    "transfer: more than 8192 coarse nodes on a non-bigraph level");
        plan = plan_transfer(shape, s.Nc, sw);
        if (plan.lazy) counts = zeroed<int>(ctx, 6);
        if (!s.small_done) amg_rowmax(ctx, A, s.maxrow, s.diag);
        amg_prolong_classical(ctx, dst, A, o, plan, s, counts, &P);
    }
    // Ac = Pro'*A*Pro, evaluated left to right                               transfer.m:66
    Csr Pt, T1, C;
    csr_transpose(ctx, dst, P, &Pt);
    if (plan.lazy_prod) {
        // the products' kernel choice runs on the previous hierarchy's counts of this level
        int* c3 = plan.lazy ? counts : zeroed<int>(ctx, 6);
        Csr Pe = P, Pte = Pt;
        if (plan.lazy) Pe.nnz = Pte.nnz = std::max(1, std::min(hint[0], P.nnz));   // (estimates for the heuristic only)
        csr_spgemm(ctx, T1out ? dst : tmp, Pte, A, &T1, c3 + 1, nullptr, c3 + 4);
        Csr T1e = T1;
        T1e.nnz = std::max(1, std::min(hint[1], T1.nnz));
        LazyPost post;   // the level's counts ride back on the last compaction
        post.src = c3;
        post.n = 5;
        csr_spgemm(ctx, dst, T1e, Pe, &C, c3 + 2, &post, nullptr, hint[3]);
        int h3[5] = {0, 0, 0, 0, 0};
        if (post.box)
            ctx->mailbox_wait(post.ticket, h3, sizeof(h3));
        else
            ctx->fetch(c3, h3, 5);
        hint[3] = h3[4];
        // P, P'A and Ac were sized by bounds (P.nnz, T1.nnz, C.nnz until here); a count outside [0, bound] is a
        // scan that never completed (a ScanTail total of -1, ipd_internal.h) and must size nothing that follows
        if (plan.lazy) spgemm_check_lazy_count(P, h3[0], "P", level);
        spgemm_check_lazy_count(T1, h3[1], "P'*A", level);
        spgemm_check_lazy_count(C, h3[2], "P'*A*P", level);
        if (plan.lazy) {
            P.nnz = Pt.nnz = h3[0];
            IPD_REQUIRE(h3[3] == 0, IPD_E_UNSUPPORTED,
                        "transfer: bigph level 1 needs a diagonal Aff block (transfer.m:20-21)");
        }
        T1.nnz = h3[1];
        C.nnz = h3[2];
    } else {
        csr_spgemm(ctx, T1out ? dst : tmp, Pt, A, &T1);
        csr_spgemm(ctx, dst, T1, P, &C);
    }
    if (hint) {
        hint[0] = P.nnz;
        hint[1] = T1.nnz;
        hint[2] = C.nnz;
    }
    if (T1out) *T1out = T1;
    *Ac = C;
    *Pout = P;
    *Ptout = Pt;
}

// ---------------------------------------------------------------------------
// hierarchy                                           (AMG/Class_AMG.m:20-85)
// ---------------------------------------------------------------------------
AmgOpts amg_fill_defaults(const ipd_amg_opts* in) {
    AmgOpts o;  // Class_AMG.m:26-34 empty-field defaults
    if (!in) return o;
    if (in->retol >= 0) o.retol = in->retol;
    if (in->bigph >= 0) o.bigph = in->bigph;
    if (in->maxit >= 0) o.maxit = in->maxit;
    if (in->theta >= 0) o.theta = in->theta;
    if (in->smoth >= 0) o.smoth = in->smoth;
    if (in->cycle >= 0) o.cycle = in->cycle;
    if (in->isnsp >= 0) o.isnsp = in->isnsp;
    if (in->inter >= 0) o.inter = in->inter;
    o.fnode = in->fnode;
    return o;
}

// twogrid_bigph.m:6-15: nargin/empty-field defaults differ from Class_AMG's
AmgOpts amg_fill_twogrid_defaults(const ipd_amg_opts* in) {
    AmgOpts o;
    o.retol = 0.0;
    o.maxit = 50;
    o.smoth = 3;
    o.isnsp = 0;
    if (in) {
        if (in->retol >= 0) o.retol = in->retol;
        if (in->maxit >= 0) o.maxit = in->maxit;
        if (in->smoth >= 0) o.smoth = in->smoth;
        if (in->isnsp >= 0) o.isnsp = in->isnsp;
        o.fnode = in->fnode;
    }
    o.bigph = 1;
    o.cycle = 'v';       // two levels: a V cycle is twogrid_it (:55-84)
    o.twogrid = true;
    o.pcg_maxit = 100;   // :72
    return o;
}

// 1 + fix(size(A,1)^(1/3)) in floating point (Class_AMG.m:76)
int amg_coarsest_threshold(int N) { return 1 + (int)std::floor(std::pow((double)N, 1.0 / 3.0)); }

// `donor`: a hierarchy of the SAME matrix and options set up earlier (AMG4POT's first right-hand
// side, Class2/AMG4POT.m:46-47).  The reference sets up twice; the two hierarchies are equal up
// to and including A_2 -- only mis_set (levels >= 2) consumes random numbers -- so that part is
// shared and the rest is built with the stream's next numbers exactly as a full setup would:
// same bits, same rand consumption, without the most expensive product of the setup.
ipd_amg* amg_setup(ipd_ctx* ctx, const Csr& A, const AmgOpts& o, ipd_rng* rng,
                   const std::shared_ptr<ipd_amg>& donor_in) {
    // a donor that itself took its levels 1-2 from another hierarchy: share with that root, so
    // that a chain of Newton steps with the same system keeps two hierarchies alive, not all
    const std::shared_ptr<ipd_amg> donor = donor_in && donor_in->donor ? donor_in->donor : donor_in;
    IPD_REQUIRE(A.nr == A.nc && A.nr > 0, IPD_E_ARG, "Class_AMG: A must be square and non-empty");
    if (o.bigph)  // Class_AMG.m:36-40
        IPD_REQUIRE(o.fnode > 0, IPD_E_ARG, "amg_options.bigph = 1 requires Nf > 0");
    IPD_REQUIRE(o.smoth >= 0 && o.maxit >= 0, IPD_E_ARG, "negative smoth/maxit");
    ctx->zreset();   // one memset for all the zero-initialised temporaries of the previous build
    std::unique_ptr<ipd_amg> h(new ipd_amg());
    h->ctx = ctx;
    h->arena.reset(new Arena(&ctx->pool));
    h->opts = o;
    h->L.resize(2);
    h->J = 1;
    const int thr = amg_coarsest_threshold(A.nr);
    // Levels 1-2 of a bigraph hierarchy depend on A and on bigph / fnode / isnsp / inter only
    // (transfer.m:19-25 draws no random numbers and uses no theta; Rk{1}, Rk{2} use none of the
    // options): exactly what is compared here, so a donor built under another theta, smoth, cycle,
    // retol or maxit is still the same levels 1-2.
    const bool share = donor && o.bigph && !o.twogrid && donor->J >= 2 && donor->opts.bigph &&
                       !donor->opts.twogrid && donor->opts.fnode == o.fnode &&
                       donor->opts.isnsp == o.isnsp && donor->opts.inter == o.inter &&
                       donor->L[1].A.nr == A.nr && donor->L[1].A.nnz == A.nnz && A.nr > thr &&
                       donor->ctx->device == ctx->device;
    if (share) {
        h->donor = donor;
        h->L[1].A = donor->L[1].A;
        h->L[1].N = A.nr;
        Level nl;
        nl.A = donor->L[2].A;
        nl.P = donor->L[2].P;
        nl.Pt = donor->L[2].Pt;
        nl.T1 = donor->L[2].T1;
        nl.cmask = donor->L[2].cmask;
        nl.N = nl.A.nr;
        h->L.push_back(nl);
        h->J = 2;
    } else {
        csr_copy(ctx, *h->arena, A, &h->L[1].A);
        h->L[1].N = A.nr;
    }
    auto more = [&] {   // Class_AMG.m:76; twogrid_bigph.m builds exactly one coarse level
        return o.twogrid ? h->J < 2 : h->L[h->J].A.nr > thr;
    };
    if (o.twogrid) IPD_REQUIRE(A.nr >= 2, IPD_E_ARG, "twogrid needs at least 2 nodes");
    while (more()) {
        IPD_REQUIRE(h->J < 40, IPD_E_NUMERIC, "Class_AMG: coarsening stalled (40 levels)");
        const Csr& Ak = h->L[h->J].A;
        Level nl;
        nl.cmask = h->arena->alloc<uint8_t>((size_t)Ak.nr);
        amg_transfer(ctx, *h->arena, Ak, o, h->J, rng, &nl.A, &nl.P, &nl.Pt, nl.cmask, &nl.T1);
        nl.N = nl.A.nr;
        IPD_REQUIRE(nl.N < Ak.nr, IPD_E_NUMERIC,
                    "Class_AMG: coarsening made no progress (the reference would loop forever)");
        h->L.push_back(nl);
        h->J += 1;
    }
    amg_prepare_levels(h.get());
    return h.release();
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ipd_transfer(ipd_ctx* ctx, const ipd_csc* A, const ipd_amg_opts* o, int level,
                            ipd_rng* rng, ipd_csc_out* Ac, ipd_csc_out* Pro, uint8_t* indC) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && A && Ac && Pro, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        AmgOpts opts = amg_fill_defaults(o);
        Arena out(&ctx->pool);
        Csr a, c, p, pt;
        // true rows of A (= transpose of the CSC arrays): a product like Q0*H0*Q0 is symmetric
        // only up to the last bit, and the setup must see exactly MATLAB's rows
        csr_upload_from_csc(ctx, out, A, false, &a);
        uint8_t* cmask = out.alloc<uint8_t>((size_t)a.nr);
        amg_transfer(ctx, out, a, opts, level, rng, &c, &p, &pt, cmask);
        csr_download_as_csc(ctx, c, false, Ac);
        csr_download_as_csc(ctx, pt, true, Pro);  // CSR of Pro' == CSC of Pro
        if (indC) ctx->fetch(cmask, indC, (size_t)a.nr);
        ctx->sync();
    });
}

extern "C" int ipd_amg_setup_dev(ipd_ctx* ctx, const ipd_dmat* A, const ipd_amg_opts* o,
                                 ipd_rng* rng, ipd_amg** out) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && A && out, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        *out = amg_setup(ctx, A->m, amg_fill_defaults(o), rng);
    });
}

extern "C" int ipd_amg_setup(ipd_ctx* ctx, const ipd_csc* A, const ipd_amg_opts* o, ipd_rng* rng,
                             ipd_amg** out) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && A && out, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        Arena up(&ctx->pool);
        Csr a;
        csr_upload_from_csc(ctx, up, A, false, &a);  // true rows (see ipd_transfer)
        *out = amg_setup(ctx, a, amg_fill_defaults(o), rng);
        ctx->sync();
    });
}

static int twogrid_host(ipd_ctx* ctx, const ipd_csc* A, const double* b, const double* guess,
                        const AmgOpts& ao, ipd_rng* rng, double* x, int32_t* it, double* rel_res,
                        double* rel_resk, double* rhok) {
    ipd_amg* h = nullptr;
    int rc = ipd_guard([&] {
        IPD_REQUIRE(ctx && A && b && x, IPD_E_ARG, "NULL argument");
        CallScope scope(ctx);
        Arena up(&ctx->pool);
        Csr a;
        csr_upload_from_csc(ctx, up, A, false, &a);
        h = amg_setup(ctx, a, ao, rng);
        ctx->sync();
    });
    if (rc != IPD_OK) return rc;
    rc = ipd_amg_solve(h, b, guess, x, it, rel_res, rel_resk, rhok);
    ipd_amg_destroy(h);
    return rc;
}
// [x,it,rel_res,rel_resk,rhok] = twogrid_bigph(A,b,amg_options)      AMG/twogrid_bigph.m:1
extern "C" int ipd_twogrid_bigph(ipd_ctx* ctx, const ipd_csc* A, const double* b,
                                 const double* guess, const ipd_amg_opts* o, double* x, int32_t* it,
                                 double* rel_res, double* rel_resk, double* rhok) {
    return twogrid_host(ctx, A, b, guess, amg_fill_twogrid_defaults(o), nullptr, x, it, rel_res,
                        rel_resk, rhok);
}
// [x,it,rel_res,rel_resk,rhok] = twogrid(A,b,amg_options)                  AMG/twogrid.m:1
extern "C" int ipd_twogrid(ipd_ctx* ctx, const ipd_csc* A, const double* b, const double* guess,
                           const ipd_amg_opts* o, ipd_rng* rng, double* x, int32_t* it,
                           double* rel_res, double* rel_resk, double* rhok) {
    AmgOpts ao = amg_fill_twogrid_defaults(o);
    ao.bigph = (o && o->bigph >= 0) ? o->bigph : 0;                       // twogrid.m:12
    ao.theta = 0.25;                                                      // mis_set(A,1/4), :50
    ao.inter = 1;
    if (ao.bigph && ao.fnode <= 0) {                                      // :24-26
        ipd_set_error("bigph = 1 requires fnode > 0");
        return IPD_E_ARG;
    }
    if (!ao.bigph && !rng) {
        ipd_set_error("twogrid: mis_set needs a rand stream");
        return IPD_E_ARG;
    }
    return twogrid_host(ctx, A, b, guess, ao, rng, x, it, rel_res, rel_resk, rhok);
}

extern "C" void ipd_amg_destroy(ipd_amg* h) {
    if (!h) return;
    if (h->ctx) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
    }
    delete h;
}

extern "C" int ipd_amg_num_levels(const ipd_amg* h) { return h ? h->J : IPD_E_ARG; }

extern "C" int ipd_amg_level_dims(const ipd_amg* h, int k, int64_t* rows, int64_t* nnz) {
    if (!h || k < 1 || k > h->J) return IPD_E_ARG;
    if (rows) *rows = h->L[k].A.nr;
    if (nnz) *nnz = h->L[k].A.nnz;
    return IPD_OK;
}

extern "C" int ipd_amg_get_A(const ipd_amg* h, int k, ipd_csc_out* A) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && A && k >= 1 && k <= h->J, IPD_E_ARG, "bad level");
        CallScope scope(h->ctx);
        csr_download_as_csc(h->ctx, h->L[k].A, false, A);
    });
}

extern "C" int ipd_amg_get_P(const ipd_amg* h, int k, ipd_csc_out* P) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && P && k >= 2 && k <= h->J, IPD_E_ARG, "bad level (Prok{k} exists for k>=2)");
        CallScope scope(h->ctx);
        csr_download_as_csc(h->ctx, h->L[k].Pt, true, P);
    });
}

extern "C" int ipd_amg_get_cmask(const ipd_amg* h, int k, uint8_t* isC) {
    return ipd_guard([&] {
        IPD_REQUIRE(h && isC && k >= 2 && k <= h->J, IPD_E_ARG, "bad level");
        CallScope scope(h->ctx);
        h->ctx->fetch(h->L[k].cmask, isC, (size_t)h->L[k - 1].A.nr);
    });
}
