// chain_corr_kernels.hpp -- the lagged sums behind thin_corr (mce_chain_corr_dev, capi_corr.hpp) for a chain that is already on the
// device.  The rule is chain_corr.hpp's; this file arranges it into passes.  fp64 throughout, no atomics, plain C++ stores only; every
// sum is formed in an order that the sizes alone fix, so two runs give the same bits.
//
//   corr_ends_kernel         the prefix sum of trunc(w) at the last row of every part (the host derives the units from it)
//   corr_mean_tile_kernel    (a) per chunk of kCorrMeanRows rows of a part and per column: sum of trunc(w) y (or of y: row units), min, max
//   corr_mean_final_kernel   (a) per part and column: the chunks in chunk order -> the centring value (chain_corr.hpp: corr_mean)
//   corr_lag_kernel          (b) a workgroup owns one CHUNK of a part (tiles of kCorrTile = 256 units, in tile order), one group of
//                            kCorrCols = 8 columns and one window of kCorrWin = 128 lags [t0, t0 + 128).  Per tile it stages the centred
//                            tile y[u0 .. u0 + 256) and the shifted strip y[u0 + t0 .. u0 + t0 + 384) in LDS -- two arrays, so that the halo
//                            does not depend on t0 -- with zeros past the part's end (a masked pair adds +0).  The row of a unit is looked
//                            up once per staged unit: 1024 prefix sums from the row where the previous tile ended (the chunk's first tile: from a
//                            galloping search by one lane) go to LDS and every lane searches there (a row of weight 5000 spans many tiles; a
//                            strip that crosses more than 1024 rows -- rows of weight 0 -- searches in memory).  A lane owns 4 consecutive
//                            lags of one column (32 lanes x 4 lags, 8 columns = 256 threads) and slides along the tile: per unit one
//                            broadcast read of y[u] and ONE new 8-byte read of the strip serve 4 FMAs.  The strip is kept as 4 phase
//                            arrays (element i at [i & 3][i >> 2]), so that the 32 lanes of a column read consecutive doubles: no bank
//                            conflict within a 32-lane half.  The chunk's sums go to partial[chunk][column][lag].
//   corr_reduce_kernel       (c) S_j(t) = the partials in chunk order
//   corr_scan_kernel         (c) rho over the window, then one lane per column: cut and running length (chain_corr.hpp: corr_advance)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_corr.hpp"
#include "chain_prep_kernels.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kCorrThreads = 256;
constexpr int kCorrTile = 256;                                  // units per tile
constexpr int kCorrLagsPerLane = 4;
constexpr int kCorrLagLanes = 32;
constexpr int kCorrWin = kCorrLagLanes * kCorrLagsPerLane;      // lags per workgroup: 128
constexpr int kCorrCols = kCorrThreads / kCorrLagLanes;         // columns per workgroup: 8
constexpr int kCorrStrip = kCorrTile + kCorrWin;                // 384
constexpr int kCorrTileStride = kCorrTile + 2;                  // doubles per column of the tile array
constexpr int kCorrPhaseLen = kCorrStrip / 4 + 4;               // entries per phase array (the last read is index kCorrStrip / 4)
constexpr int kCorrCache = 1024;                                // prefix sums kept in LDS per strip
constexpr int kCorrMeanRows = 1024;                             // rows per chunk of the mean pass
constexpr int kCorrMaxDim = 127;

struct CorrPart {
    const double* rows;      // first row of the part
    int64_t first, nrows;    // its rows in the concatenated numbering
    int64_t units, c_base;   // units of its series; prefix sum of trunc(w) before its first row
    int64_t chunk0;          // its first chunk of the lag pass
    int32_t tiles_per_chunk, pad;
    int64_t mchunk0;         // its first chunk of the mean pass
};

// per column, carried from window to window and read back after each
struct CorrState {
    long long cut;
    double sum, s0;
};

// the part that owns chunk k (parts[p].chunk0 ascending from 0; mean = the mean pass's numbering)
__device__ __forceinline__ int corr_part_of(const CorrPart* __restrict__ parts, int nparts, int64_t k, bool mean)
{
    return mce_seg::last_at_or_below(nparts, k, [parts, mean](int i) { return mean ? parts[i].mchunk0 : parts[i].chunk0; });
}

__global__ __launch_bounds__(kCorrThreads) void corr_ends_kernel(const PrepPart* __restrict__ parts, int nparts, const long long* __restrict__ c,
                                                                 long long* __restrict__ ends)
{
    const int p = blockIdx.x * kCorrThreads + threadIdx.x;
    if (p < nparts) ends[p] = c[parts[p].first + parts[p].nrows - 1];
}

// grid: the mean chunks.  Thread (rs, j): column j of the rows rs, rs + RS, .. of the chunk, RS = 256 / CL row lanes, CL = the power of
// two >= ndim; then the RS lanes of a column in lane order.  out[chunk][j] = {sum, min, max}.
__global__ __launch_bounds__(kCorrThreads) void corr_mean_tile_kernel(const CorrPart* __restrict__ parts, int nparts, int64_t ncols, int iw, int itheta,
                                                                      int ndim, int cl, int integer, double* __restrict__ out)
{
    __shared__ double s_sum[kCorrThreads], s_lo[kCorrThreads], s_hi[kCorrThreads];
    const int tid = threadIdx.x, j = tid % cl, rs = tid / cl, nrs = kCorrThreads / cl;
    const int64_t chunk = blockIdx.x;
    const int p = corr_part_of(parts, nparts, chunk, true);
    const CorrPart part = parts[p];
    const int64_t r0 = (chunk - part.mchunk0) * kCorrMeanRows;
    const int64_t r1 = r0 + kCorrMeanRows < part.nrows ? r0 + kCorrMeanRows : part.nrows;
    double sum = 0.0, lo = INFINITY, hi = -INFINITY;
    if (j < ndim)
        for (int64_t r = r0 + rs; r < r1; r += nrs) {
            const double* row = part.rows + r * ncols;
            const double wt = integer ? (double)mce_prep::weight_int(row[iw]) : 1.0;
            if (wt > 0.0) {
                const double v = row[itheta + j];
                sum += wt * v;
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
        }
    s_sum[tid] = sum; s_lo[tid] = lo; s_hi[tid] = hi;
    __syncthreads();
    if (rs == 0 && j < ndim) {
        for (int k = 1; k < nrs; ++k) {
            sum += s_sum[k * cl + j];
            lo = s_lo[k * cl + j] < lo ? s_lo[k * cl + j] : lo;
            hi = s_hi[k * cl + j] > hi ? s_hi[k * cl + j] : hi;
        }
        double* o = out + (chunk * ndim + j) * 3;
        o[0] = sum; o[1] = lo; o[2] = hi;
    }
}

// one thread per (part, column): the part's chunks in order
__global__ __launch_bounds__(kCorrThreads) void corr_mean_final_kernel(const CorrPart* __restrict__ parts, int nparts, int ndim, const double* __restrict__ tiles,
                                                                       double* __restrict__ mean)
{
    const int64_t e = (int64_t)blockIdx.x * kCorrThreads + threadIdx.x;
    if (e >= (int64_t)nparts * ndim) return;
    const int p = (int)(e / ndim), j = (int)(e - (int64_t)p * ndim);
    const CorrPart part = parts[p];
    const int64_t nch = (part.nrows + kCorrMeanRows - 1) / kCorrMeanRows;
    double sum = 0.0, lo = INFINITY, hi = -INFINITY;
#pragma unroll 8
    for (int64_t k = 0; k < nch; ++k) {
        const double* t = tiles + ((part.mchunk0 + k) * ndim + j) * 3;
        sum += t[0];
        lo = t[1] < lo ? t[1] : lo;
        hi = t[2] > hi ? t[2] : hi;
    }
    mean[e] = part.units > 0 ? mce_corr::corr_mean(sum, lo, hi, part.units) : 0.0;
}

// the first i in [lo, n) with c[i] >= target, galloping up from lo (c never decreases; target <= c[n - 1])
__device__ __forceinline__ int64_t corr_gallop(const long long* __restrict__ c, int64_t n, int64_t lo, long long target)
{
    int64_t hi = lo, step = 1;
    while (hi < n - 1 && c[hi] < target) {
        lo = hi + 1;
        hi = hi + step < n - 1 ? hi + step : n - 1;
        step <<= 1;
    }
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (c[mid] >= target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

struct CorrShared {
    double tile[kCorrCols * kCorrTileStride];
    double strip[kCorrCols * 4 * kCorrPhaseLen];
    long long cache[kCorrCache];
    long long hint[2];
};

// Stage `len` units from unit `ustart` of the part (columns j0 .. j0 + kCorrCols of the measured ones, centred; zeros past the part's end
// and for columns >= ndim) into the tile array (which = 0) or the phase arrays of the strip (which = 1).  Every thread of the block calls it.
// s.hint[which]: a row at or before the row of unit `ustart`, where the window of prefix sums kept in LDS starts.  In the first tile of a
// chunk (`first`) one lane finds it by a galloping search; every call leaves the next call's hint, the row it found for the next
// call's first unit (the strip) or for the unit before that (the tile); `next`: how many units further on the next call starts.
// Barriers: s.cache and s.hint are shared by the tile's and the strip's call, and lanes search s.cache until they leave the call.  So
// every call OPENS with a barrier -- no lane refills the window while another still searches the previous call's --, a second one
// separates the refill from the searches, and the caller puts one between the last call and the sums and one after the sums.  The
// hint is read by every lane between the first two barriers and written (by one lane) only after the second.
__device__ __forceinline__ void corr_stage(CorrShared& s, const CorrPart& part, const long long* __restrict__ cpart, int integer, int64_t ncols, int itheta,
                                           int ndim, int j0, const double* __restrict__ mean_p, int64_t ustart, int len, int which, bool first, int next)
{
    const int tid = threadIdx.x;
    const bool lookup = integer && ustart < part.units;
    __syncthreads();                                   // (the previous call's searches of s.cache are over)
    if (first) {
        if (lookup && tid == 0) s.hint[which] = corr_gallop(cpart, part.nrows, 0, part.c_base + ustart + 1);
        __syncthreads();
    }
    const int64_t rlo = lookup ? s.hint[which] : 0;
    int ncache = 0;
    if (lookup) {
        ncache = part.nrows - rlo < kCorrCache ? (int)(part.nrows - rlo) : kCorrCache;
        for (int i = tid; i < ncache; i += kCorrThreads) s.cache[i] = cpart[rlo + i];
    }
    __syncthreads();
    // the unit whose row is the next call's hint: the next call's first unit, or (the tile: len == next) the unit before it
    const int xhint = next < len ? next : len - 1;
    for (int x = tid; x < len; x += kCorrThreads) {
        const int64_t u = ustart + x;
        const double* row = nullptr;
        if (u < part.units) {
            int64_t r = u;
            if (integer) {
                const long long target = part.c_base + u + 1;
                if (s.cache[ncache - 1] >= target) {
                    int lo = 0, hi = ncache - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (s.cache[mid] >= target) hi = mid;
                        else lo = mid + 1;
                    }
                    r = rlo + lo;
                } else {
                    r = corr_gallop(cpart, part.nrows, rlo + ncache, target);
                }
                if (x == xhint) s.hint[which] = r;
            }
            row = part.rows + r * ncols + itheta;
        }
#pragma unroll
        for (int k = 0; k < kCorrCols; ++k) {
            const int j = j0 + k;
            const double v = (row && j < ndim) ? row[j] - mean_p[j] : 0.0;
            if (which == 0) s.tile[k * kCorrTileStride + x] = v;
            else s.strip[(k * 4 + (x & 3)) * kCorrPhaseLen + (x >> 2)] = v;
        }
    }
}

// grid: (chunks, column groups, windows of kCorrWin lags from tau0); partial[(chunk * ndim + j) * nlag + z * kCorrWin + lag]
__global__ __launch_bounds__(kCorrThreads) void corr_lag_kernel(const CorrPart* __restrict__ parts, int nparts, const long long* __restrict__ c, int integer,
                                                                int64_t ncols, int itheta, int ndim, const double* __restrict__ mean, int64_t tau0,
                                                                int nlag, double* __restrict__ partial)
{
    __shared__ CorrShared s;
    const int tid = threadIdx.x, g = tid % kCorrLagLanes, k = tid / kCorrLagLanes;
    const int64_t chunk = blockIdx.x;
    const int j0 = blockIdx.y * kCorrCols;
    const int64_t t0 = tau0 + (int64_t)blockIdx.z * kCorrWin;
    const int p = corr_part_of(parts, nparts, chunk, false);
    const CorrPart part = parts[p];
    const long long* cpart = c + part.first;
    const double* mean_p = mean + (int64_t)p * ndim;
    const int64_t ntiles = (part.units + kCorrTile - 1) / kCorrTile;
    const int64_t tile0 = (chunk - part.chunk0) * part.tiles_per_chunk;
    const int64_t tile1 = tile0 + part.tiles_per_chunk < ntiles ? tile0 + part.tiles_per_chunk : ntiles;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    const double* a = s.tile + k * kCorrTileStride;
    const double* b = s.strip + (k * 4) * kCorrPhaseLen + g;
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t u0 = tile * kCorrTile;
        corr_stage(s, part, cpart, integer, ncols, itheta, ndim, j0, mean_p, u0, kCorrTile, 0, tile == tile0, kCorrTile);
        corr_stage(s, part, cpart, integer, ncols, itheta, ndim, j0, mean_p, u0 + t0, kCorrStrip, 1, tile == tile0, kCorrTile);
        __syncthreads();
        // lane (k, g): lags t0 + 4 g + {0, 1, 2, 3}; b_i = strip[u + 4 g + i]
        double b0 = b[0], b1 = b[kCorrPhaseLen], b2 = b[2 * kCorrPhaseLen], b3 = b[3 * kCorrPhaseLen];
#pragma unroll 4
        for (int u = 0; u < kCorrTile; u += 4) {
            const int m = (u >> 2) + 1;
            const double a0 = a[u], a1 = a[u + 1], a2 = a[u + 2], a3 = a[u + 3];
            const double n0 = b[m], n1 = b[kCorrPhaseLen + m], n2 = b[2 * kCorrPhaseLen + m], n3 = b[3 * kCorrPhaseLen + m];
            acc0 += a0 * b0; acc1 += a0 * b1; acc2 += a0 * b2; acc3 += a0 * b3;
            acc0 += a1 * b1; acc1 += a1 * b2; acc2 += a1 * b3; acc3 += a1 * n0;
            acc0 += a2 * b2; acc1 += a2 * b3; acc2 += a2 * n0; acc3 += a2 * n1;
            acc0 += a3 * b3; acc1 += a3 * n0; acc2 += a3 * n1; acc3 += a3 * n2;
            b0 = n0; b1 = n1; b2 = n2; b3 = n3;
        }
        __syncthreads();
    }
    if (j0 + k < ndim) {
        double* o = partial + (chunk * ndim + j0 + k) * nlag + (int64_t)blockIdx.z * kCorrWin + g * kCorrLagsPerLane;
        o[0] = acc0; o[1] = acc1; o[2] = acc2; o[3] = acc3;
    }
}

// S[(tau0 + lag) * ndim + j] = partial[0 .. nchunks)[j][lag] in chunk order; one thread per (j, lag)
__global__ __launch_bounds__(kCorrThreads) void corr_reduce_kernel(const double* __restrict__ partial, int64_t nchunks, int ndim, int nlag, int64_t tau0,
                                                                   double* __restrict__ S)
{
    const int64_t e = (int64_t)blockIdx.x * kCorrThreads + threadIdx.x;
    if (e >= (int64_t)ndim * nlag) return;
    const int j = (int)(e / nlag), lag = (int)(e - (int64_t)j * nlag);
    double sum = 0.0;
#pragma unroll 8
    for (int64_t ch = 0; ch < nchunks; ++ch) sum += partial[(ch * ndim + j) * nlag + lag];
    S[(tau0 + lag) * ndim + j] = sum;
}

// one block: rho_j(t) for the lags tau0 .. tau1 (tau1 <= cap) by all threads, then lane j walks column j in ascending lag: its cut and
// running sum
__global__ __launch_bounds__(kCorrThreads) void corr_scan_kernel(const double* __restrict__ S, const double* __restrict__ n_tau, int ndim, int64_t tau0,
                                                                 int64_t tau1, double min_corr, double* __restrict__ rho, CorrState* __restrict__ state)
{
    const int64_t count = (tau1 - tau0 + 1) * ndim;
    for (int64_t e = threadIdx.x; e < count; e += kCorrThreads) {
        const int64_t t = tau0 + e / ndim;
        const int jj = (int)(e % ndim);
        rho[t * ndim + jj] = t == 0 ? 1.0 : mce_corr::corr_rho(S[t * ndim + jj], n_tau[t], S[jj], n_tau[0]);
    }
    __syncthreads();
    const int j = threadIdx.x;
    if (j >= ndim) return;
    mce_corr::CorrColumn col;
    const double s0 = S[j];
    if (tau0 > 0) { col.cut = state[j].cut; col.sum = state[j].sum; }
    for (int64_t t = tau0 > 0 ? tau0 : 1; t <= tau1; ++t) mce_corr::corr_advance(col, t, rho[t * ndim + j], min_corr);
    state[j].cut = col.cut;
    state[j].sum = col.sum;
    state[j].s0 = s0;
}

}  // namespace mce
