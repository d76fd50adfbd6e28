// The KKT operators' interface (ipd_kkt.hip: Ax, Aty, invAAt, invHHt; ipd_asat.hip: ASAt) for their callers
// (ipd_pot.hip, ipd_driver.hip, ipd_apd_warm.hip), and the frame the two units' C ABI entries share.
// All asynchronous on ctx->stream; ASAt reads its entry count back.
#pragma once

#include <initializer_list>
#include <utility>

#include "ipd_internal.h"
#include "ipd_kkt_plan.h"

void kkt_ax(ipd_ctx* ctx, const double* x, const double* p, const double* q, int m, int n, double* y);
void kkt_aty(ipd_ctx* ctx, const double* y, const double* p, const double* q, int m, int n, double* z);
void kkt_asat(ipd_ctx* ctx, Arena& dst, const uint8_t* s, const double* p, const double* q, int m, int n, Csr* H);
void kkt_inv_aat(ipd_ctx* ctx, const double* x, const double* p, const double* q, int m, int n, double sg1, double sg2,
                 double* y);
void kkt_inv_hht(ipd_ctx* ctx, const double* v, const double* p, const double* q, int m, int n, double sg,
                 const double* phi, double* y);
// invHHt with l = Ax(phi) and the partial sums of ||phi||^2 hoisted out (kkt_phi_consts -> npart): both depend on
// the problem only, while the warm start calls invHHt once per iteration (warmup_class2.m:72)
void kkt_inv_hht_pre(ipd_ctx* ctx, const double* v, const double* p, const double* q, int m, int n, double sg,
                     const double* l, const double* part, int npart, double* y);
int kkt_phi_consts(ipd_ctx* ctx, const double* phi, const double* p, const double* q, int m, int n, double* l,
                   double* part /* phi_parts(m, n) doubles */);

static inline void kkt_require(const KktDimCheck& c) { if (c.code != IPD_OK) throw IpdError(c.code, c.msg); }

// ---- the C ABI's frames ---------------------------------------------------------------------------
// a *_dev entry: NULL check, dimension check, scope, then call(m, n) on the caller's device pointers
template <class F>
static inline int kkt_dev_entry(ipd_ctx* ctx, bool pointers_ok, int64_t m, int64_t n, F&& call) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && pointers_ok, IPD_E_ARG, "NULL argument");
        kkt_require(kkt_check_mn(m, n));
        CallScope scope(ctx);
        call((int)m, (int)n);
    });
}

// a host entry: the same, with the operands, then p and q, copied to scratch; call(d, dp, dq, dy, m, n) runs on the
// copies d[k], dp, dq and a scratch result of ny doubles, which is fetched into out (ny = 0: the call delivers its
// result itself)
using KktOperand = std::pair<const void*, size_t>;   // host pointer, bytes
template <class F>
static inline int kkt_host_entry(ipd_ctx* ctx, std::initializer_list<KktOperand> ops, const double* p, const double* q,
                                 int64_t m, int64_t n, void* out, size_t ny, F&& call) {
    bool ok = p && q && out;
    for (const KktOperand& o : ops) ok = ok && o.first;
    return kkt_dev_entry(ctx, ok, m, n, [&](int mi, int ni) {
        auto up = [&](const void* host, size_t bytes) {
            void* dev = ctx->scratch->alloc<uint8_t>(bytes);
            ctx->upload_bytes(dev, host, bytes);
            return dev;
        };
        const void* d[2] = {nullptr, nullptr};
        int k = 0;
        for (const KktOperand& o : ops) d[k++] = up(o.first, o.second);
        const double* dp = static_cast<const double*>(up(p, sizeof(double) * mi));
        const double* dq = static_cast<const double*>(up(q, sizeof(double) * ni));
        double* dy = ny ? ctx->scratch->alloc<double>(ny) : nullptr;
        call(d, dp, dq, dy, mi, ni);
        if (ny) ctx->fetch(dy, static_cast<double*>(out), ny);
    });
}
