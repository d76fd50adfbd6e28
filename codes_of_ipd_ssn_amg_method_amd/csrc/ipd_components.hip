// Connected components on the device                                   (components.m:32-55)
//
// The labels are found by a concurrent union-find; the O(N) bookkeeping that turns them into
// blocks/sizes/p/r and applies an injected order is host logic (components_from_roots, ipd_hybrid_plan.h).
#pragma clang fp contract(off)

#include "ipd_hybrid_state.h"

#include <algorithm>

// Concurrent union-find over the whole chip (the scheme of Jaiganesh & Burtscher's ECL-CC):
// parent[x] <= x always; every edge (i,j), j < i, merges the two trees by hooking the LARGER
// root under the smaller with a compare-and-swap, retrying from the returned value when another
// wave got there first; a last pass points every node at its root.  The root of a tree is the
// smallest member of the component whatever the interleaving, so the labels are deterministic.
// Three launches and no rounds: the single-workgroup hook-and-compress loop this replaces took
// 350-400 us per Newton step at m = n = 4096.
__device__ __forceinline__ int cc_root(int x, int* __restrict__ parent) {
    int curr = parent[x];
    if (curr != x) {
        int prev = x, next;
        while (curr > (next = parent[curr])) {   // path halving: only ever points further up
            parent[prev] = next;
            prev = curr;
            curr = next;
        }
    }
    return curr;
}

__device__ __forceinline__ void cc_union(int a, int b, int* __restrict__ parent) {
    int ra = cc_root(a, parent), rb = cc_root(b, parent);
    while (ra != rb) {
        if (ra < rb) {
            const int t = ra;
            ra = rb;
            rb = t;
        }
        const int seen = atomicCAS(&parent[ra], ra, rb);   // ra > rb: hook ra under rb
        if (seen == ra) break;
        ra = seen;                                          // ra was hooked meanwhile: follow it
    }
}

__global__ __launch_bounds__(256) void k_cc_init(int N, const int* __restrict__ rp,
                                                 const int* __restrict__ ci,
                                                 int* __restrict__ parent) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        int first = i;   // rows are sorted: the first entry is the smallest neighbour
        if (rp[i] < rp[i + 1]) first = min(i, ci[rp[i]]);
        parent[i] = first;
    }
}

__global__ __launch_bounds__(256) void k_cc_hook(int N, const int* __restrict__ rp,
                                                 const int* __restrict__ ci,
                                                 int* __restrict__ parent) {
    // rows of up to 32 entries: one thread each; longer rows (hubs, dense masks): one wave each
    const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gsz = gridDim.x * blockDim.x;
    for (int i = gtid; i < N; i += gsz) {
        const int b = rp[i], e = rp[i + 1];
        if (e - b > 32) continue;
        for (int t = b; t < e; ++t) {
            const int j = ci[t];
            if (j >= i) break;
            cc_union(i, j, parent);
        }
    }
    const int lane = threadIdx.x & 63;
    for (int i = gtid >> 6; i < N; i += gsz >> 6) {
        const int b = rp[i], e = rp[i + 1];
        if (e - b <= 32) continue;
        for (int t = b + lane; t < e; t += 64) {
            const int j = ci[t];
            if (j < i) cc_union(i, j, parent);
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_flatten(int N, const int* __restrict__ parent,
                                                    int* __restrict__ root_out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        int r = parent[i];
        while (true) {
            const int up = parent[r];
            if (up == r) break;
            r = up;
        }
        root_out[i] = r;
    }
}

void find_components(ipd_ctx* ctx, const Csr& A, Components* out) {
    IPD_REQUIRE(A.nr == A.nc, IPD_E_ARG, "Adjacency matrix must be square");  // components.m:33
    const int N = A.nr;
    int* parent = ctx->scratch->alloc<int>((size_t)N);
    int* root = ctx->scratch->alloc<int>((size_t)N);
    const int g = std::max(1, std::min((N + 255) / 256, 1024));
    hipLaunchKernelGGL(k_cc_init, dim3(g), dim3(256), 0, ctx->stream, N, A.rp, A.ci, parent);
    // a wave per long row needs 64 threads per row to keep the chip busy
    const int gh = std::max(1, std::min((N + 3) / 4, 2048));
    hipLaunchKernelGGL(k_cc_hook, dim3(gh), dim3(256), 0, ctx->stream, N, A.rp, A.ci, parent);
    hipLaunchKernelGGL(k_cc_flatten, dim3(g), dim3(256), 0, ctx->stream, N, parent, root);
    IPD_KERNEL_CHECK();
    std::vector<int> par((size_t)N);
    ctx->fetch(root, par.data(), (size_t)N);
    const std::vector<int>& ord = ctx->comp_order;   // injected by ipd_ctx_set_component_order, or empty
    const CompError e = components_from_roots(par.data(), N, ord.data(), (int)ord.size(), out);
    IPD_REQUIRE(e == COMP_OK, e == COMP_BAD_ROOT ? IPD_E_NUMERIC : IPD_E_ARG, comp_error_text(e));
}

// One-shot: the order applies to the NEXT top-level call that visits components on this context
// (components, Hybrid_AMG, AMG4POT and their two-grid / PCG variants) and is cleared when that
// call returns.  order == NULL or ncomp == 0 clears it.
extern "C" int ipd_ctx_set_component_order(ipd_ctx* ctx, const int64_t* smallest_members, int64_t ncomp) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && ncomp >= 0 && ncomp < (int64_t(1) << 30), IPD_E_ARG, "bad argument");
        ctx->comp_order.clear();
        if (smallest_members)
            for (int64_t k = 0; k < ncomp; ++k) ctx->comp_order.push_back((int)smallest_members[k]);
    });
}

extern "C" int ipd_components(ipd_ctx* ctx, const ipd_csc* A, int64_t* blocks, int64_t* sizes,
                              int64_t* p, int64_t* r, int64_t* ncomp) {
    return ipd_guard([&] {
        IPD_REQUIRE(ctx && A && blocks && sizes && p && r && ncomp, IPD_E_ARG, "NULL argument");
        IPD_REQUIRE(A->nrows == A->ncols, IPD_E_ARG, "Adjacency matrix must be square");
        CallScope scope(ctx);
        CompOrderScope order_scope(ctx);
        Csr a;
        csr_upload_from_csc(ctx, *ctx->scratch, A, true, &a);  // undirected graph: pattern symmetric
        Components cc;
        find_components(ctx, a, &cc);
        *ncomp = cc.ncomp;
        for (int i = 0; i < a.nr; ++i) {
            blocks[i] = cc.blocks[(size_t)i];
            p[i] = cc.p[(size_t)i];
        }
        for (int c = 0; c < cc.ncomp; ++c) sizes[c] = cc.sizes[(size_t)c];
        for (int c = 0; c <= cc.ncomp; ++c) r[c] = cc.r[(size_t)c];
    });
}
