// The convergence block and the one-workgroup Jacobi-PCG of the coarsest level: device code that the launch path
// (k_pcg, k_fused: ipd_cycle.hip) and the single-workgroup interpreter (ipd_interp.h) both run.
#pragma once

#include "ipd_cycle_args.h"

__device__ __forceinline__ void conv_block(const ConvArgs& a, double* red) {
    double s = 0.0;
    for (int k0 = threadIdx.x; k0 < a.n; k0 += 4 * BT) {  // 4 independent loads in flight
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + u * BT;
            v[u] = a.r[k < a.n ? k : a.n - 1];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s += (k0 + u * BT < a.n) ? v[u] * v[u] : 0.0;
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) {
        double* hist = a.hist;
        const double res = sqrt(tot);
        if (a.first) {
            hist[0] = res;
            hist[1] = res;
            hist[2] = res;
            hist[3] = 1.0;
            hist[4] = 0.0;
        } else {
            const double prev = hist[1];
            hist[2] = prev;
            hist[1] = res;
            hist[3] = res / hist[0];
            hist[4] = res / prev;
        }
    }
}

// A 1x1 coarsest level (dense masks: levels 2048 / 1024 / 1) through the block-wide reductions
// costs ~10 us per cycle for five multiplications; one thread runs the same recurrence in
// registers.  Every block sum of the general path has a single nonzero term here, so the bits
// are the same.
__device__ __forceinline__ void pcg_single(const PcgArgs& a) {
    if (threadIdx.x == 0) {
        double h = 0.0;   // H(1,1); a structurally empty row leaves it 0 as the general path does
        for (int t = a.rp[0]; t < a.rp[1]; ++t)
            if (a.ci[t] == 0) h = a.va[t];
        const double g0 = a.guess ? a.guess[0] : 0.0;
        double r = a.rhs[0] - (a.guess ? h * g0 : 0.0);                         // :68
        double p = a.precd == 2 ? r / h : r;
        double d = g0;
        double delta_new = r * p;
        const double delta_0 = delta_new, thresh = a.tol * a.tol * delta_0;
        long long it = 0;
        while (it < a.maxit && delta_new > thresh) {                            // :76
            const double delta_old = delta_new;
            const double q = h * p;
            const double alpha = delta_old / (q * p);                           // :78
            d += alpha * p;
            r = r - alpha * q;                                                  // :79
            const double w = a.precd == 2 ? r / h : r;                          // :80
            delta_new = r * w;                                                  // :81
            p = w + (delta_new / delta_old) * p;                                // :82-83
            ++it;
            if (a.out && it <= a.nresk) a.out[1 + it] = sqrt(fabs(delta_new / delta_0));
        }
        a.d[0] = d;
        if (a.out) {
            a.out[0] = (double)it;
            a.out[1] = sqrt(fabs(delta_new / delta_0));
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void pcg_block(const PcgArgs& a, double* red) {
    if (a.N == 1) {
        pcg_single(a);
        return;
    }
    const int tid = threadIdx.x;
    const int N = a.N, L = a.L, gpb = BT / L;
    const int g = tid / L, gl = tid - g * L;
    double* r = a.work;
    double* p = a.work + N;
    double* q = a.work + 2 * (size_t)N;
    double* dg = a.work + 3 * (size_t)N;
    const int niter = (N + gpb - 1) / gpb;
    // r = e - H*d0 ; diag ; p = M^-1 r ; delta_new = r'p                     :68-70
    double acc = 0.0;
    for (int it = 0; it < niter; ++it) {
        const int row = it * gpb + g;
        const bool valid = row < N;
        double s = 0.0, dd = 0.0;
        if (valid)
            for (int t = a.rp[row] + gl; t < a.rp[row + 1]; t += L) {
                const int j = a.ci[t];
                if (a.guess) s += a.va[t] * a.guess[j];
                if (j == row) dd = a.va[t];
            }
        s = group_sum(s, L, red);
        dd = group_sum(dd, L, red);
        if (valid && gl == 0) {
            const double ri = a.rhs[row] - s;
            const double pi = a.precd == 2 ? ri / dd : ri;
            r[row] = ri;
            dg[row] = dd;
            p[row] = pi;
            a.d[row] = a.guess ? a.guess[row] : 0.0;
            acc += ri * pi;
        }
    }
    double delta_new = block_sum(acc, red);
    const double delta_0 = delta_new;
    const double thresh = a.tol * a.tol * delta_0;
    long long it_count = 0;
    while (it_count < a.maxit && delta_new > thresh) {                          // :76
        const double delta_old = delta_new;
        __syncthreads();
        acc = 0.0;
        for (int it = 0; it < niter; ++it) {  // q = H*p ; q'p
            const int row = it * gpb + g;
            const bool valid = row < N;
            double s = 0.0;
            if (valid)
                for (int t = a.rp[row] + gl; t < a.rp[row + 1]; t += L) s += a.va[t] * p[a.ci[t]];
            s = group_sum(s, L, red);
            if (valid && gl == 0) {
                q[row] = s;
                acc += s * p[row];
            }
        }
        const double qp = block_sum(acc, red);
        const double alpha = delta_old / qp;                                    // :78
        acc = 0.0;
        for (int row = tid; row < N; row += BT) {
            a.d[row] += alpha * p[row];
            const double ri = r[row] - alpha * q[row];                          // :79
            r[row] = ri;
            const double wi = a.precd == 2 ? ri / dg[row] : ri;                 // :80
            q[row] = wi;  // q is free again: holds w
            acc += ri * wi;
        }
        delta_new = block_sum(acc, red);                                        // :81
        const double beta = delta_new / delta_old;                              // :82
        for (int row = tid; row < N; row += BT) p[row] = q[row] + beta * p[row];  // :83
        ++it_count;
        if (tid == 0 && a.out && it_count <= a.nresk)
            a.out[1 + it_count] = sqrt(fabs(delta_new / delta_0));              // :85
    }
    if (tid == 0 && a.out) {
        a.out[0] = (double)it_count;
        a.out[1] = sqrt(fabs(delta_new / delta_0));                             // :87 (0/0 -> NaN)
    }
    __syncthreads();
}
