// chain_prep_kernels.hpp -- burn-in, concatenation, thinning, the s1/s2 split, the column split and the fs / SumW reductions of a
// chain that is already on the device (mce_chain_weights_dev .. mce_chain_reduce_dev, capi_prep.hpp).  The per-row rules are
// chain_prep.hpp's; this file only arranges them into passes.
//
// The burned chains stay where the reader left them: a small table (PrepPart: pointer, first row, row count) maps row g of the
// concatenated numbering to its buffer.  Spans: a TILE is kPrepTile = 512 rows (256 threads x 2 rows); the single-block scan
// takes kPrepScanThreads = 256 tiles per round (131 072 rows) and carries a running sum from round to round.
//   weights     prep_weights_kernel   the weight column gathered into one vector w[n]
//               prep_tile_kernel      per tile: sum and max of trunc(w), sum of w - trunc(w), count of refused weights
//               prep_scan_kernel      exclusive int64 sums of the tile sums (one block) and the total
//               prep_totals_kernel    max / fractional sum / refused count over the tiles, one block, fixed order
//               prep_cum_kernel       c[i]: inclusive int64 prefix sum of trunc(w)
//   select      prep_flag_kernel      integer rule, factor >= max: cand[i] = i or -1
//               prep_bin_kernel       bin rule: one wave per bin, cand[b] = first row of maximal weight or -1
//               prep_count_kernel, prep_scan_kernel, prep_fill_kernel     compaction of cand -> src / new_w (count, then fill)
//               prep_search_kernel    integer rule, factor < max: one binary search in c per output row
//   gather      prep_gather_kernel    one lane per (output row, column): source row src[rows[r]], 8-byte loads that neighbouring
//                                     lanes make contiguous (a row of 23 or 29 doubles is 16-byte aligned only every other row)
//   reduce      prep_like_tile_kernel, prep_like_final_kernel, prep_fs_kernel   max(logL), SumW, fs = logL - max: callers of prep_like_tile /
//               prep_like_final / prep_logl, which reduce one SEGMENT of rows; the farm's per-root kernels (chain_farm_kernels.hpp) call them too
// Every sum is formed in an order that depends on the sizes only (serial per thread, then a shared-memory tree), never with
// floating-point atomics, so two runs give the same bits.  All indices are 64-bit; plain C++ stores only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_kernels.hpp"
#include "chain_prep.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kPrepThreads = 256;
constexpr int kPrepRowsPerThread = 2;
constexpr int64_t kPrepTile = (int64_t)kPrepThreads * kPrepRowsPerThread;
constexpr int kPrepScanThreads = 256;

struct PrepPart {
    const double* rows;
    int64_t first, nrows;
};

// totals as the device writes them (mce_prep::WeightTotals, plus the compaction's count)
struct PrepTotals {
    long long sum_int, max_int, bad, n_out;
    double frac;
};

// row g of the concatenated numbering (0 <= g < n; parts are non-empty, parts[0].first = 0, firsts ascending)
__device__ __forceinline__ const double* prep_row(const PrepPart* __restrict__ parts, int nparts, int64_t g, int64_t ncols)
{
    const int lo = mce_seg::last_at_or_below(nparts, g, [parts](int i) { return parts[i].first; });
    return parts[lo].rows + (g - parts[lo].first) * ncols;
}

__global__ __launch_bounds__(kPrepThreads) void prep_weights_kernel(const PrepPart* __restrict__ parts, int nparts, int64_t n, int64_t ncols, int iw,
                                                                    double* __restrict__ w)
{
    for (int64_t i = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPrepThreads)
        w[i] = prep_row(parts, nparts, i, ncols)[iw];
}

// inclusive scan of one int64 per thread over the block (Hillis-Steele in shared memory); every thread must call it
__device__ __forceinline__ long long prep_block_scan(long long v, long long* s, int tid)
{
    s[tid] = v;
    __syncthreads();
    for (int off = 1; off < kPrepThreads; off <<= 1) {
        const long long add = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += add;
        __syncthreads();
    }
    const long long r = s[tid];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kPrepThreads) void prep_tile_kernel(const double* __restrict__ w, int64_t n, int64_t ntiles, long long* __restrict__ tile_sum,
                                                                 long long* __restrict__ tile_max, double* __restrict__ tile_frac,
                                                                 long long* __restrict__ tile_bad)
{
    __shared__ long long s_sum[kPrepThreads], s_max[kPrepThreads], s_bad[kPrepThreads];
    __shared__ double s_frac[kPrepThreads];
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long long sum = 0, mx = 0, bad = 0;
        double frac = 0.0;
#pragma unroll
        for (int k = 0; k < kPrepRowsPerThread; ++k) {
            const int64_t i = tile * kPrepTile + (int64_t)tid * kPrepRowsPerThread + k;
            if (i < n) {
                const double v = w[i];
                if (!mce_prep::weight_ok(v)) ++bad;
                const long long wi = mce_prep::weight_int(v);
                sum += wi;
                mx = wi > mx ? wi : mx;
                frac += mce_prep::weight_frac(v);
            }
        }
        s_sum[tid] = sum; s_max[tid] = mx; s_bad[tid] = bad; s_frac[tid] = frac;
        __syncthreads();
        for (int off = kPrepThreads / 2; off > 0; off >>= 1) {
            if (tid < off) {
                s_sum[tid] += s_sum[tid + off];
                s_max[tid] = s_max[tid + off] > s_max[tid] ? s_max[tid + off] : s_max[tid];
                s_bad[tid] += s_bad[tid + off];
                s_frac[tid] += s_frac[tid + off];
            }
            __syncthreads();
        }
        if (tid == 0) { tile_sum[tile] = s_sum[0]; tile_max[tile] = s_max[0]; tile_bad[tile] = s_bad[0]; tile_frac[tile] = s_frac[0]; }
        __syncthreads();
    }
}

// out[t] = in[0] + .. + in[t-1], *total = the sum of all; ONE block of kPrepScanThreads (= kPrepThreads) threads
__global__ __launch_bounds__(kPrepScanThreads) void prep_scan_kernel(const long long* __restrict__ in, int64_t nt, long long* __restrict__ out,
                                                                     long long* __restrict__ total)
{
    static_assert(kPrepScanThreads == kPrepThreads, "prep_block_scan is written for kPrepThreads");
    __shared__ long long s[kPrepThreads];
    const int tid = threadIdx.x;
    long long carry = 0;
    for (int64_t base = 0; base < nt; base += kPrepScanThreads) {
        const int64_t t = base + tid;
        const long long v = t < nt ? in[t] : 0;
        const long long incl = prep_block_scan(v, s, tid);
        if (t < nt) out[t] = carry + incl - v;
        s[tid] = incl;
        __syncthreads();
        carry += s[kPrepThreads - 1];
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

__global__ __launch_bounds__(kPrepThreads) void prep_totals_kernel(const long long* __restrict__ tile_max, const double* __restrict__ tile_frac,
                                                                   const long long* __restrict__ tile_bad, int64_t nt, PrepTotals* __restrict__ tot)
{
    __shared__ long long s_max[kPrepThreads], s_bad[kPrepThreads];
    __shared__ double s_frac[kPrepThreads];
    const int tid = threadIdx.x;
    long long mx = 0, bad = 0;
    double frac = 0.0;
    for (int64_t t = tid; t < nt; t += kPrepThreads) {
        mx = tile_max[t] > mx ? tile_max[t] : mx;
        bad += tile_bad[t];
        frac += tile_frac[t];
    }
    s_max[tid] = mx; s_bad[tid] = bad; s_frac[tid] = frac;
    __syncthreads();
    for (int off = kPrepThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s_max[tid] = s_max[tid + off] > s_max[tid] ? s_max[tid + off] : s_max[tid];
            s_bad[tid] += s_bad[tid + off];
            s_frac[tid] += s_frac[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) { tot->max_int = s_max[0]; tot->bad = s_bad[0]; tot->frac = s_frac[0]; }
}

__global__ __launch_bounds__(kPrepThreads) void prep_cum_kernel(const double* __restrict__ w, int64_t n, int64_t ntiles, const long long* __restrict__ tile_base,
                                                                long long* __restrict__ c)
{
    __shared__ long long s[kPrepThreads];
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long long v[kPrepRowsPerThread], mine = 0;
#pragma unroll
        for (int k = 0; k < kPrepRowsPerThread; ++k) {
            const int64_t i = tile * kPrepTile + (int64_t)tid * kPrepRowsPerThread + k;
            v[k] = i < n ? mce_prep::weight_int(w[i]) : 0;
            mine += v[k];
        }
        long long run = tile_base[tile] + prep_block_scan(mine, s, tid) - mine;
#pragma unroll
        for (int k = 0; k < kPrepRowsPerThread; ++k) {
            const int64_t i = tile * kPrepTile + (int64_t)tid * kPrepRowsPerThread + k;
            run += v[k];
            if (i < n) c[i] = run;
        }
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_flag_kernel(const long long* __restrict__ c, int64_t n, long long factor, long long* __restrict__ cand)
{
    for (int64_t i = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPrepThreads)
        cand[i] = mce_prep::int_keep_flag(i ? c[i - 1] : 0, c[i], factor, i == 0) ? i : -1;
}

// one wave per bin (b = 1 .. nedges): lanes stride over the bin's rows, then the 64 candidates are compared in lane order
__global__ __launch_bounds__(kPrepThreads) void prep_bin_kernel(const double* __restrict__ w, int64_t n, const double* __restrict__ edges, int64_t nedges,
                                                                long long* __restrict__ cand)
{
    __shared__ double s_w[kPrepThreads];
    __shared__ long long s_i[kPrepThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kPrepThreads / 64;
    const int64_t rounds = (nedges + (int64_t)gridDim.x * kWaves - 1) / ((int64_t)gridDim.x * kWaves);
    for (int64_t r = 0; r < rounds; ++r) {          // (every thread takes every round: the barriers below are block-wide)
        const int64_t b = 1 + (r * gridDim.x + blockIdx.x) * kWaves + wave;
        double bw = 0.0;
        long long bi = -1;
        if (b <= nedges) {
            int64_t lo, hi;
            mce_prep::bin_range(edges, nedges, b, n, &lo, &hi);
            for (int64_t i = lo + lane; i < hi; i += 64) {
                const double v = w[i];
                if (mce_prep::bin_better(v, i, bw, bi)) { bw = v; bi = i; }
            }
        }
        s_w[tid] = bw;
        s_i[tid] = bi;
        __syncthreads();
        if (lane == 0 && b <= nedges) {
            for (int l = 1; l < 64; ++l)
                if (s_i[tid + l] >= 0 && mce_prep::bin_better(s_w[tid + l], s_i[tid + l], bw, bi)) { bw = s_w[tid + l]; bi = s_i[tid + l]; }
            cand[b - 1] = bi;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_count_kernel(const long long* __restrict__ cand, int64_t len, int64_t ntiles, long long* __restrict__ tile_cnt)
{
    __shared__ long long s[kPrepThreads];
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long long cnt = 0;
#pragma unroll
        for (int k = 0; k < kPrepRowsPerThread; ++k) {
            const int64_t i = tile * kPrepTile + (int64_t)tid * kPrepRowsPerThread + k;
            if (i < len && cand[i] >= 0) ++cnt;
        }
        const long long incl = prep_block_scan(cnt, s, tid);
        if (tid == kPrepThreads - 1) tile_cnt[tile] = incl;
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_fill_kernel(const long long* __restrict__ cand, int64_t len, int64_t ntiles, const long long* __restrict__ tile_obase,
                                                                 const double* __restrict__ w, int integer, int64_t n_out, long long* __restrict__ src,
                                                                 double* __restrict__ new_w)
{
    __shared__ long long s[kPrepThreads];
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        long long v[kPrepRowsPerThread], cnt = 0;
#pragma unroll
        for (int k = 0; k < kPrepRowsPerThread; ++k) {
            const int64_t i = tile * kPrepTile + (int64_t)tid * kPrepRowsPerThread + k;
            v[k] = i < len ? cand[i] : -1;
            if (v[k] >= 0) ++cnt;
        }
        long long o = tile_obase[tile] + prep_block_scan(cnt, s, tid) - cnt;
#pragma unroll
        for (int k = 0; k < kPrepRowsPerThread; ++k)
            if (v[k] >= 0) {
                if (o < n_out) {
                    src[o] = v[k];
                    new_w[o] = integer ? (double)mce_prep::weight_int(w[v[k]]) : w[v[k]];
                }
                ++o;
            }
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_search_kernel(const long long* __restrict__ c, int64_t n, long long factor, int64_t n_out,
                                                                   const double* __restrict__ w, long long* __restrict__ src, double* __restrict__ new_w)
{
    for (int64_t m = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; m < n_out; m += (int64_t)gridDim.x * kPrepThreads) {
        const int64_t i = mce_prep::int_lower_bound(reinterpret_cast<const int64_t*>(c), n, (m + 1) * factor);
        src[m] = i;
        new_w[m] = (double)mce_prep::weight_int(w[i]);
    }
}

// Output row r, column col: k = rows ? rows[r] : r indexes the thinned chain (n_thin rows), g = src ? src[k] : k the burned,
// concatenated one (n rows).  An index outside its range writes NaN and reads nothing.
__global__ __launch_bounds__(kPrepThreads) void prep_gather_kernel(const PrepPart* __restrict__ parts, int nparts, int64_t n, int64_t ncols, int iw, int ilike,
                                                                   int itheta, const long long* __restrict__ src, const double* __restrict__ new_w,
                                                                   int64_t n_thin, const long long* __restrict__ rows, int64_t n_out,
                                                                   double* __restrict__ params, double* __restrict__ w_out, double* __restrict__ like_out,
                                                                   double* __restrict__ full)
{
    const int64_t total = n_out * ncols, nparam = ncols - itheta;
    for (int64_t e = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kPrepThreads) {
        const int64_t r = e / ncols;
        const int col = (int)(e - r * ncols);
        const int64_t k = rows ? rows[r] : r;
        double v = __builtin_nan("");
        if (k >= 0 && k < n_thin) {
            const int64_t g = src ? src[k] : k;
            if (g >= 0 && g < n) v = (col == iw && new_w) ? new_w[k] : prep_row(parts, nparts, g, ncols)[col];
        }
        if (full) full[e] = v;
        if (params && col >= itheta) params[r * nparam + (col - itheta)] = v;
        if (w_out && col == iw) w_out[r] = v;
        if (like_out && col == ilike) like_out[r] = v;
    }
}

// ---- the like / fs reduction of one SEGMENT of rows: the whole chain here, one root of a wave in chain_farm_kernels.hpp -------------
// The order of every sum is fixed by the segment's own size: serial over a thread's 2 rows, a tree over the block from off = 128
// down, and in the final pass strided by 256 over the segment's tiles and the same tree again.
struct PrepLikeShared {
    double mx[kPrepThreads], sum[kPrepThreads];
    long long bad[kPrepThreads];          // NaN likelihoods in the low 32 bits, weights that are not finite above them
};

__device__ __forceinline__ double prep_logl(double like, int pos_lnp) { return pos_lnp ? like : -like; }

// max, sum and packed bad count over the block's threads -> s.mx[0], s.sum[0], s.bad[0]; every thread of the block calls it
__device__ __forceinline__ void prep_like_tree(PrepLikeShared& s, int tid, double mx, double sum, long long bad)
{
    s.mx[tid] = mx; s.sum[tid] = sum; s.bad[tid] = bad;
    __syncthreads();
    for (int off = kPrepThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            s.mx[tid] = s.mx[tid + off] > s.mx[tid] ? s.mx[tid + off] : s.mx[tid];
            s.sum[tid] += s.sum[tid + off];
            s.bad[tid] += s.bad[tid + off];
        }
        __syncthreads();
    }
}

// Tile `tile` of a segment of n rows (like, w: its first row): max(logL) (NaNs are counted, not compared), sum of w, counts of NaN logL
// and of weights that are not finite -> *t_max, *t_sum, *t_bad.  Every thread of the block; the closing barrier frees s for the next tile.
__device__ __forceinline__ void prep_like_tile(PrepLikeShared& s, const double* __restrict__ like, const double* __restrict__ w, int64_t n, int64_t tile,
                                               int pos_lnp, double* __restrict__ t_max, double* __restrict__ t_sum, long long* __restrict__ t_bad)
{
    const int tid = threadIdx.x;
    double mx = -INFINITY, sum = 0.0;
    long long bad = 0;
#pragma unroll
    for (int k = 0; k < kPrepRowsPerThread; ++k) {
        const int64_t i = tile * kPrepTile + (int64_t)tid * kPrepRowsPerThread + k;
        if (i < n) {
            const double l = prep_logl(like[i], pos_lnp), v = w[i];
            if (l != l) bad += 1;
            else mx = l > mx ? l : mx;
            if (!(v - v == 0.0)) bad += (1ll << 32);
            sum += v;
        }
    }
    prep_like_tree(s, tid, mx, sum, bad);
    if (tid == 0) { *t_max = s.mx[0]; *t_sum = s.sum[0]; *t_bad = s.bad[0]; }
    __syncthreads();
}

// The nt tiles of a segment (t_*: its first) -> out[0] = max(logL), out[1] = SumW, out[2] = NaN likelihoods, out[3] = weights that are
// not finite.  Every thread of ONE block; a caller with a next segment puts a barrier before it.
__device__ __forceinline__ void prep_like_final(PrepLikeShared& s, const double* __restrict__ t_max, const double* __restrict__ t_sum,
                                                const long long* __restrict__ t_bad, int64_t nt, double* __restrict__ out)
{
    const int tid = threadIdx.x;
    double mx = -INFINITY, sum = 0.0;
    long long bad = 0;
    for (int64_t t = tid; t < nt; t += kPrepThreads) {
        mx = t_max[t] > mx ? t_max[t] : mx;
        sum += t_sum[t];
        bad += t_bad[t];
    }
    prep_like_tree(s, tid, mx, sum, bad);
    if (tid == 0) {
        out[0] = s.mx[0];
        out[1] = s.sum[0];
        out[2] = (double)(s.bad[0] & 0xFFFFFFFFll);
        out[3] = (double)(s.bad[0] >> 32);
    }
}

__global__ __launch_bounds__(kPrepThreads) void prep_like_tile_kernel(const double* __restrict__ like, const double* __restrict__ w, int64_t n, int64_t ntiles,
                                                                      int pos_lnp, double* __restrict__ tile_max, double* __restrict__ tile_sumw,
                                                                      long long* __restrict__ tile_bad)
{
    __shared__ PrepLikeShared s;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x)          // (the same trips for every thread of the block: the barriers inside)
        prep_like_tile(s, like, w, n, tile, pos_lnp, tile_max + tile, tile_sumw + tile, tile_bad + tile);
}

// one block
__global__ __launch_bounds__(kPrepThreads) void prep_like_final_kernel(const double* __restrict__ tile_max, const double* __restrict__ tile_sumw,
                                                                       const long long* __restrict__ tile_bad, int64_t nt, double* __restrict__ out)
{
    __shared__ PrepLikeShared s;
    prep_like_final(s, tile_max, tile_sumw, tile_bad, nt, out);
}

__global__ __launch_bounds__(kPrepThreads) void prep_fs_kernel(const double* __restrict__ like, int64_t n, int pos_lnp, const double* __restrict__ red,
                                                               double* __restrict__ fs)
{
    const double mx = red[0];
    for (int64_t i = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kPrepThreads)
        fs[i] = prep_logl(like[i], pos_lnp) - mx;
}

// the reader's host patches, written into a device array: vals[list[i].token] = patch[i]
__global__ __launch_bounds__(kPrepThreads) void prep_patch_kernel(const ChainPatch* __restrict__ list, const double* __restrict__ patch, int64_t nlist,
                                                                  int64_t ntok, double* __restrict__ vals)
{
    for (int64_t i = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; i < nlist; i += (int64_t)gridDim.x * kPrepThreads) {
        const int64_t t = list[i].token;
        if (t >= 0 && t < ntok) vals[t] = patch[i];
    }
}

}  // namespace mce
