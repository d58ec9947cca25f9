// density_order.hpp -- step 6 of param_marginals.hpp (the densities of a grid in the order of mar_before, their running sums, the cut of a
// probability) as one workgroup of kRedThreads threads does it on arrays in LDS.  mar_hpd_kernel (param_marginals_kernels.hpp) runs it
// on the G points of a column, con_region_kernel (param_contours_kernels.hpp) on the G * G cells of a pair.  mar_before is a strict total
// order, so the sorted arrays are the serial drivers' std::sort, and the running sums are formed by ONE thread in that order: the bits of
// a cut do not depend on the network.
#pragma once

#include <hip/hip_runtime.h>

#include "block_reduce.hpp"
#include "param_marginals.hpp"

namespace mce {

// the bitonic network on mar_before over the n pairs (s_rho[q], s_k[q]), n a power of two.  Every thread of the workgroup calls it; the
// pairs are written and a __syncthreads() is behind them when it begins, and it ends behind one
__device__ __forceinline__ void order_sort(double* s_rho, int* s_k, int n)
{
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int a = threadIdx.x; a < n; a += kRedThreads) {
                const int b = a ^ stride;
                if (b > a) {
                    const bool up = (a & size) == 0;             // this pair ends in the order of step 6
                    const double ra = s_rho[a], rb = s_rho[b];
                    const int ka = s_k[a], kb = s_k[b];
                    const bool b_first = mce_mar::mar_before(rb, kb, ra, ka);
                    if (b_first == up) { s_rho[a] = rb; s_rho[b] = ra; s_k[a] = kb; s_k[b] = ka; }
                }
            }
            __syncthreads();
        }
    }
}

// the running sums of the sorted pairs, s_cum[q] = term(s_rho[0], s_k[0]) + .. + term(s_rho[q], s_k[q]), by the ONE thread that calls it
template <class Term> __device__ __forceinline__ void order_running_sum(const double* s_rho, const int* s_k, int n, double* s_cum, Term term)
{
    double run = 0.0;
    for (int q = 0; q < n; ++q) { run += term(s_rho[q], s_k[q]); s_cum[q] = run; }
}
// the same of the densities as they stand
__device__ __forceinline__ void order_running_sum(const double* s_rho, int n, double* s_cum)
{
    double run = 0.0;
    for (int q = 0; q < n; ++q) { run += s_rho[q]; s_cum[q] = run; }
}

// the first position whose running sum reaches the target (none does: the last position), in every thread.  `red`: block_min's words
__device__ __forceinline__ int order_cut(const double* s_cum, int n, double target, double* red)
{
    double first = (double)(n - 1);
    for (int q = threadIdx.x; q < n; q += kRedThreads)
        if (s_cum[q] >= target && (double)q < first) first = (double)q;
    return (int)block_min(first, red);
}

}  // namespace mce
