// block_reduce.hpp -- the workgroup reductions of the statistics kernels, for workgroups of kRedThreads = 256 threads (four waves of
// 64).  Every one is a fixed tree: shuffles inside a wave, one LDS word per wave, then the four waves in wave order -- so a result
// depends on the values and their threads alone, never on the dispatch.  Each opens with a __syncthreads() before it writes its LDS
// words and has one behind the write, so the same words may serve call after call.  "Valid in thread 0" means what it says: the other
// threads hold something else.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mce {

constexpr int kRedThreads = 256;
constexpr int kRedWaves = kRedThreads / 64;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// the extreme of a wave, in lane 0: before(u, v) says that u replaces v (a NaN never wins a comparison)
template <class Before> __device__ __forceinline__ double wave_pick(double v, Before before)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { const double u = __shfl_down(v, o, 64); v = before(u, v) ? u : v; }
    return v;
}
__device__ __forceinline__ double wave_min(double v) { return wave_pick(v, [](double u, double w) { return u < w; }); }
__device__ __forceinline__ double wave_max(double v) { return wave_pick(v, [](double u, double w) { return u > w; }); }

// sum over the workgroup; result valid in thread 0.  `red` = kRedWaves doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < kRedWaves; ++i) s += red[i];
    }
    return s;
}

// the extreme of the workgroup, valid in every thread: the waves' extremes in wave order
template <class Before> __device__ __forceinline__ double block_pick(double v, double* red, Before before)
{
    v = wave_pick(v, before);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = red[0];
    for (int i = 1; i < kRedWaves; ++i) s = before(red[i], s) ? red[i] : s;
    return s;
}
__device__ __forceinline__ double block_min(double v, double* red) { return block_pick(v, red, [](double u, double w) { return u < w; }); }
__device__ __forceinline__ double block_max(double v, double* red) { return block_pick(v, red, [](double u, double w) { return u > w; }); }

// maximum and "a NaN was seen" over the workgroup; result valid in thread 0.  fmax drops NaNs, so they travel in the flag.
__device__ __forceinline__ void block_max_nan(double& m, int& nan, double* red_m, int* red_n)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        m = fmax(m, __shfl_down(m, o, 64));
        nan |= __shfl_down(nan, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { red_m[w] = m; red_n[w] = nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < kRedWaves; ++i) { m = fmax(m, red_m[i]); nan |= red_n[i]; }
    }
}

// OR over the workgroup, valid in every thread.  `red64` = kRedWaves words of LDS.
__device__ __forceinline__ unsigned long long block_or(unsigned long long v, unsigned long long* red64)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red64[wv] = v;
    __syncthreads();
    unsigned long long m = 0;
#pragma unroll
    for (int i = 0; i < kRedWaves; ++i) m |= red64[i];
    return m;
}

// the best (f, row) pair of the workgroup, in thread 0: better(f2, row2, f, row) says that the first pair beats the second.  bf, br:
// kRedWaves entries of LDS each.
template <class Better> __device__ __forceinline__ void block_best(double& f, long long& row, double* bf, long long* br, Better better)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double uf = __shfl_down(f, o, 64);
        const long long ur = __shfl_down(row, o, 64);
        if (better(uf, ur, f, row)) { f = uf; row = ur; }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { bf[w] = f; br[w] = row; }
    __syncthreads();
    if (threadIdx.x == 0) {
        f = bf[0];
        row = br[0];
        for (int i = 1; i < kRedWaves; ++i)
            if (better(bf[i], br[i], f, row)) { f = bf[i]; row = br[i]; }
    }
}

// one workgroup folds an array of per-tile sums: tot[j] = the sum over k < nt of src[k * stride + j], j < NS.  Thread t adds the
// entries k = t, t + 256, .. in turn, all NS of an entry before the next entry; then NS block_sums in index order.  Valid in thread 0.
template <int NS> __device__ __forceinline__ void block_fold(const double* __restrict__ src, int64_t nt, int64_t stride, double* tot, double* red)
{
    double acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = 0.0;
    for (int64_t k = threadIdx.x; k < nt; k += kRedThreads)
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] += src[k * stride + j];
#pragma unroll
    for (int j = 0; j < NS; ++j) tot[j] = block_sum(acc[j], red);
}

}  // namespace mce
