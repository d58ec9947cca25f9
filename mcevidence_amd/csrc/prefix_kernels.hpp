// prefix_kernels.hpp -- the convergence batches of the estimator (reference MCEvidence.py:1034-1131 with brange / nbatch:
// ln E of the FIRST S_b rows of the chain, for B sizes) on the device.  The prefixes of a row-major chain are contiguous, so a
// batch differs from the whole chain only in its row count and in the shift max(logl[0 : p_b]) of its likelihood terms:
//   prefix_max_kernel + prefix_max_final_kernel    lmax[b] = max(logl[0 : p_b]) for all B prefixes, ONE read of logl
//   prefix_fs_kernel                               fs[i] = logl[i] - lmax[b], i < p_b  (the host's single IEEE subtraction)
//   prefix_dotp_kernel + prefix_dotp_final_kernel  cross evidence: the B reductions from the distance matrix of ONE search
// Conventions as in reduce_kernels.hpp: fixed-order trees, no floating-point atomics, results independent of dispatch order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"

namespace mce {

constexpr int kPrefixThreads = 256;
constexpr int kPrefixMaxRows = 4 * kPrefixThreads;      // rows of logl per workgroup of prefix_max_kernel
constexpr int kMaxPrefix = 256;                         // == MCE_MAX_PREFIX
static_assert(kPrefixThreads == kRedThreads, "block_sum's and block_max_nan's trees are kRedThreads wide");

// Workgroup j reads the rows [j R, min((j + 1) R, p_max)), R = kPrefixMaxRows, once, and writes for every segment
// s = [p_{s-1}, p_s) that meets them blkmax[s][j] = the maximum over the rows of both (NaN if one of them is NaN).  A segment s
// meets exactly the workgroups p_{s-1} / R .. (p_s - 1) / R, which is what the final pass reads: nothing else is ever written or
// read, so the array needs no clearing.  prefix[] is non-decreasing (the host checks it); an empty segment (p_s == p_{s-1}) has
// no entry.  The launch has ceil(p_max / R) workgroups.
__global__ __launch_bounds__(kPrefixThreads) void prefix_max_kernel(const double* __restrict__ logl, const int64_t* __restrict__ prefix, int B,
                                                                    double* __restrict__ blkmax /*[B][nblk]*/, int nblk)
{
    __shared__ int64_t sp[kMaxPrefix];
    __shared__ double red_m[kPrefixThreads / 64];
    __shared__ int red_n[kPrefixThreads / 64];
    for (int i = threadIdx.x; i < B; i += kPrefixThreads) sp[i] = prefix[i];
    __syncthreads();
    const int64_t pmax = sp[B - 1];
    const int64_t r0 = (int64_t)blockIdx.x * kPrefixMaxRows;
    if (r0 >= pmax) return;                                   // (a launch larger than the rows: the whole workgroup leaves)
    const int64_t r1 = r0 + kPrefixMaxRows < pmax ? r0 + kPrefixMaxRows : pmax;
    double v[kPrefixMaxRows / kPrefixThreads];
#pragma unroll
    for (int u = 0; u < kPrefixMaxRows / kPrefixThreads; ++u) {
        const int64_t i = r0 + (int64_t)u * kPrefixThreads + threadIdx.x;
        v[u] = i < r1 ? logl[i] : 0.0;
    }
    // the segments of the first and of the last row of the range: the smallest s with p_s > row (p_{B-1} = pmax > every row)
    int s_lo = 0, s_hi = 0;
    while (sp[s_lo] <= r0) ++s_lo;
    s_hi = s_lo;
    while (sp[s_hi] <= r1 - 1) ++s_hi;
    const double NEG_INF = -__builtin_huge_val();
    for (int s = s_lo; s <= s_hi; ++s) {
        const int64_t lo = s > 0 ? sp[s - 1] : 0, hi = sp[s];
        if (hi <= lo) continue;                               // (uniform over the workgroup)
        double m = NEG_INF;
        int nan = 0;
#pragma unroll
        for (int u = 0; u < kPrefixMaxRows / kPrefixThreads; ++u) {
            const int64_t i = r0 + (int64_t)u * kPrefixThreads + threadIdx.x;
            if (i < r1 && i >= lo && i < hi) {
                if (v[u] != v[u]) nan = 1;
                else m = fmax(m, v[u]);
            }
        }
        block_max_nan(m, nan, red_m, red_n);
        if (threadIdx.x == 0) blkmax[(int64_t)s * nblk + blockIdx.x] = nan ? __builtin_nan("") : m;
    }
}

// one workgroup: the segments in order -- a fixed tree over the segment's workgroup maxima, then the running maximum.
// lmax[b] = max(logl[0 : p_b]); NaN once a NaN lies below p_b (np.amax); -inf while every row is -inf.
__global__ __launch_bounds__(kPrefixThreads) void prefix_max_final_kernel(const double* __restrict__ blkmax, const int64_t* __restrict__ prefix, int B,
                                                                          int nblk, double* __restrict__ lmax /*[B]*/)
{
    __shared__ double red_m[kPrefixThreads / 64];
    __shared__ int red_n[kPrefixThreads / 64];
    const double NEG_INF = -__builtin_huge_val();
    double run = NEG_INF;
    int run_nan = 0;
    for (int s = 0; s < B; ++s) {
        const int64_t lo = s > 0 ? prefix[s - 1] : 0, hi = prefix[s];
        if (hi > lo) {
            const int64_t j0 = lo / kPrefixMaxRows, j1 = (hi - 1) / kPrefixMaxRows;
            double m = NEG_INF;
            int nan = 0;
            for (int64_t j = j0 + threadIdx.x; j <= j1; j += kPrefixThreads) {
                const double x = blkmax[(int64_t)s * nblk + j];
                if (x != x) nan = 1;
                else m = fmax(m, x);
            }
            block_max_nan(m, nan, red_m, red_n);
            run = fmax(run, m);                               // (meaningful in thread 0 only)
            run_nan |= nan;
        }
        if (threadIdx.x == 0) lmax[s] = run_nan ? __builtin_nan("") : run;
    }
}

// fs[i] = logl[i] - *lmax for i < p: the likelihood terms of one prefix, into the scratch the next search reads
__global__ __launch_bounds__(kPrefixThreads) void prefix_fs_kernel(const double* __restrict__ logl, int64_t p, const double* __restrict__ lmax,
                                                                   double* __restrict__ fs)
{
    const int64_t i = (int64_t)blockIdx.x * kPrefixThreads + threadIdx.x;
    if (i < p) fs[i] = logl[i] - *lmax;
}

// Cross evidence: every batch searches ALL of s2 (reference :1075), so the neighbour distances of row q do not depend on the
// batch.  dist[p_max, ld] is the distance matrix of ONE search; workgroup (j, b) sums the rows [256 j, 256 (j + 1)) below p_b:
//   partial[b][j][k] = sum_q sgn(w_q) exp(lnC_D + D ln r_qk - ln|w_q| + (logl_q - lmax_b))
// -- dotp_partial_kernel's term and sign rule, with the batch's OWN shift inside the exponent (a prefix whose rows all lie far
// below the chain's maximum keeps a finite sum).  A workgroup wholly beyond p_b writes zeros.
__global__ __launch_bounds__(kPrefixThreads) void prefix_dotp_kernel(const double* __restrict__ dist, int ld, int kmax, int D, double lnc,
                                                                     const double* __restrict__ w, const double* __restrict__ logl,
                                                                     const double* __restrict__ lmax, const int64_t* __restrict__ prefix,
                                                                     double* __restrict__ partial /*[B][nblk][kmax]*/)
{
    __shared__ double red[kRedThreads / 64];
    const int b = blockIdx.y;
    const int64_t p = prefix[b];
    double* out = partial + ((int64_t)b * gridDim.x + blockIdx.x) * kmax;
    if ((int64_t)blockIdx.x * kPrefixThreads >= p) {
        for (int k = threadIdx.x; k < kmax; k += kPrefixThreads) out[k] = 0.0;
        return;
    }
    const int64_t q = (int64_t)blockIdx.x * kPrefixThreads + threadIdx.x;
    const bool live = q < p;
    double base = 0.0, sgn = 1.0;
    if (live) {
        const double wq = w[q];
        base = lnc - log(fabs(wq)) + (logl[q] - lmax[b]);
        sgn = wq < 0.0 ? -1.0 : 1.0;
    }
    for (int k = 0; k < kmax; ++k) {
        double t = 0.0;
        if (live) {
            const double r = dist[q * (int64_t)ld + k];
            t = sgn * exp(base + (double)D * log(r));
        }
        const double s = block_sum(t, red);
        if (threadIdx.x == 0) out[k] = s;
    }
}

// final pass: workgroup (k, b) sums partial[b][:, k] in a fixed order
__global__ __launch_bounds__(kPrefixThreads) void prefix_dotp_final_kernel(const double* __restrict__ partial, int64_t nblk, int kmax,
                                                                           double* __restrict__ dotp /*[B][kmax]*/)
{
    __shared__ double red[kRedThreads / 64];
    const int k = blockIdx.x, b = blockIdx.y;
    const double* src = partial + (int64_t)b * nblk * kmax;
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < nblk; j += kPrefixThreads) acc += src[j * kmax + k];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) dotp[(int64_t)b * kmax + k] = s;
}

}  // namespace mce
