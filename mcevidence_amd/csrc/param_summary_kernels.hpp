// param_summary_kernels.hpp -- the posterior summary behind summary= (mce_param_summary_dev, capi_summary.hpp) for chains that are
// already on the device.  The rule is param_summary.hpp's; this file arranges it into launches that serve any number of systems (one
// system = one (x, ld, n, d, w, fs) segment: the s1 partition of one root) by the segment-tile scheme of seg_tiles.hpp, which states
// the invariant these launches keep; here a system's bits do not depend on the size of a sort pass either.  Plain C++ stores only.
// A RUN is one (system, column): the n values of the column with their weights.
//
//   sum_tile_kernel      per tile: sum a, sum a^2, the used rows, the rows with a bad weight / a NaN f, the (max f, lowest row) pair;
//                        per tile and column: sum a x, min, max, the rows with a value that is not finite
//   sum_sys_kernel       one workgroup per system: its tiles, thread t taking t, t + 256, .., then block reductions: W, A2, rows, best
//   sum_col_kernel       one workgroup per run: the column's tile sums in the same order: m = S / W, min, max, refused rows
//   sum_var_tile_kernel  per tile and column: sum a (x - m)^2 about the run's computed m
//   sum_var_col_kernel   one workgroup per run: v = sum / W
//   sum_keys_kernel      per element of a sort pass: the order-preserving key of x and the weight, column-major, run after run; a row
//                        that is not used gets the largest key and the weight 0: it sorts behind every used row and adds nothing
//   (rocprim::segmented_radix_sort_pairs: stable, deterministic)
//   sum_scan_tile_kernel per tile of kSumScanTile sorted elements of ONE run: the tile's total by a fixed tree
//   sum_search_kernel    one wave per run, lane t serving target t: the tile totals added in tile order until the inclusive total
//                        reaches q W, then the elements of that tile in order (param_summary.hpp: sum_search); Q = the key there
//   sum_result_kernel    one workgroup per system: the status and its precedence, and the result block
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "param_summary.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kPsumThreads = kRedThreads;
constexpr int kSumWaves = kRedWaves;
constexpr int kSumTileRows = mce_seg::kSegTileRows;
static_assert(kSumTileRows == 2 * kPsumThreads, "a thread holds two rows of its tile");
constexpr int kSumScanTile = 1024;                              // sorted elements per scan tile: 4 per thread
constexpr int kSumTileHead = 7;                                 // per tile: sum a, sum a^2, used, bad weights, bad f, best f, best row
constexpr int kSumTileCol = 4;                                  // per tile and column: sum a x, min, max, bad values
constexpr int kSumSys = 6;                                      // per system: W, A2, used, bad weights + 2 bad f, best f, best row
constexpr int kSumCol = 5;                                      // per run: m, v, min, max, bad values

struct SumSeg {
    const double* x;
    const double* w;
    const double* fs;
    int64_t ld, n;
    int64_t out_off;                                            // of the system's result block, in doubles
    int64_t col0;                                               // the system's first run
    int32_t d, pad;
};

// one run of a sort pass
struct SumRun {
    int64_t begin;                                              // first element in the pass's buffers
    int64_t tile0;                                              // first scan tile in the pass
    int32_t seg, col;
};

// grid: the tiles.  head[tile][kSumTileHead], cols[tile][kSumTileCol][dmax].  Thread t owns the rows r0 + t and r0 + t + 256 of the
// tile (a row past the tile's end, in the last tile of a segment, is treated as a row that is not used); per column the wave's 128 rows
// are combined by shuffles, the four waves in wave order.
__global__ __launch_bounds__(kPsumThreads) void sum_tile_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int dmax,
                                                               double* __restrict__ head, double* __restrict__ cols)
{
    __shared__ double red[kSumWaves];
    __shared__ double bf[kSumWaves];
    __shared__ long long br[kSumWaves];
    __shared__ double part[kSumWaves][kSumTileCol][mce_sum::kSumMaxDim + 1];
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const SumSeg g = segs[s];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ra = r0 + threadIdx.x, rb = ra + kPsumThreads;
    const double a0 = ra < r1 ? g.w[ra] : 0.0, a1 = rb < r1 ? g.w[rb] : 0.0;
    const bool u0 = mce_sum::sum_used(a0), u1 = mce_sum::sum_used(a1);
    double bestf = 0.0, badf = 0.0;
    long long bestr = -1;
    if (g.fs) {
        if (u0) { const double f = g.fs[ra]; badf += mce_sum::sum_like_bad(f) ? 1.0 : 0.0; bestf = f; bestr = ra; }
        if (u1) { const double f = g.fs[rb]; badf += mce_sum::sum_like_bad(f) ? 1.0 : 0.0; if (mce_sum::sum_better(f, rb, bestf, bestr)) { bestf = f; bestr = rb; } }
    }
    const double t[5] = {(u0 ? a0 : 0.0) + (u1 ? a1 : 0.0), (u0 ? a0 * a0 : 0.0) + (u1 ? a1 * a1 : 0.0), (u0 ? 1.0 : 0.0) + (u1 ? 1.0 : 0.0),
                         ((u0 && mce_sum::sum_weight_bad(a0)) ? 1.0 : 0.0) + ((u1 && mce_sum::sum_weight_bad(a1)) ? 1.0 : 0.0), badf};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double v = block_sum(t[k], red);
        if (threadIdx.x == 0) head[tile * kSumTileHead + k] = v;
    }
    block_best(bestf, bestr, bf, br, mce_sum::sum_better);
    if (threadIdx.x == 0) {
        head[tile * kSumTileHead + 5] = bestf;
        head[tile * kSumTileHead + 6] = (double)bestr;
    }
    const double* __restrict__ x0 = g.x + ra * g.ld;
    const double* __restrict__ x1 = g.x + rb * g.ld;
    const double INF = __builtin_huge_val();
    for (int j = 0; j < g.d; ++j) {
        double sx = 0.0, mn = INF, mx = -INF, bad = 0.0;
        if (u0) { const double v = x0[j]; sx = a0 * v; mn = v; mx = v; bad = mce_sum::sum_value_bad(v) ? 1.0 : 0.0; }
        if (u1) { const double v = x1[j]; sx += a1 * v; mn = v < mn ? v : mn; mx = v > mx ? v : mx; bad += mce_sum::sum_value_bad(v) ? 1.0 : 0.0; }
        sx = wave_sum(sx);
        mn = wave_min(mn);
        mx = wave_max(mx);
        bad = wave_sum(bad);
        if (lane == 0) { part[wv][0][j] = sx; part[wv][1][j] = mn; part[wv][2][j] = mx; part[wv][3][j] = bad; }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < g.d; j += kPsumThreads) {
        double sx = part[0][0][j], mn = part[0][1][j], mx = part[0][2][j], bad = part[0][3][j];
        for (int k = 1; k < kSumWaves; ++k) {
            sx += part[k][0][j];
            mn = part[k][1][j] < mn ? part[k][1][j] : mn;
            mx = part[k][2][j] > mx ? part[k][2][j] : mx;
            bad += part[k][3][j];
        }
        double* out = cols + tile * kSumTileCol * dmax;
        out[0 * dmax + j] = sx;
        out[1 * dmax + j] = mn;
        out[2 * dmax + j] = mx;
        out[3 * dmax + j] = bad;
    }
}

// one workgroup per system.  sys[y][kSumSys]
__global__ __launch_bounds__(kPsumThreads) void sum_sys_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, const double* __restrict__ head,
                                                              double* __restrict__ sys)
{
    __shared__ double red[kSumWaves];
    __shared__ double bf[kSumWaves];
    __shared__ long long br[kSumWaves];
    const int y = blockIdx.x;
    // (block_fold's order, written out: the best pair shares the one pass over the tiles with the five sums)
    const int64_t t0 = tile0[y], nt = mce_seg::seg_ntiles(segs[y].n);
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    double bestf = 0.0;
    long long bestr = -1;
    for (int64_t k = threadIdx.x; k < nt; k += kPsumThreads) {
        const double* h = head + (t0 + k) * kSumTileHead;
#pragma unroll
        for (int j = 0; j < 5; ++j) acc[j] += h[j];
        const long long r = (long long)h[6];
        if (mce_sum::sum_better(h[5], r, bestf, bestr)) { bestf = h[5]; bestr = r; }
    }
    double tot[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) tot[j] = block_sum(acc[j], red);
    block_best(bestf, bestr, bf, br, mce_sum::sum_better);
    if (threadIdx.x == 0) {
        double* out = sys + (int64_t)y * kSumSys;
        out[0] = tot[0];
        out[1] = tot[1];
        out[2] = tot[2];
        out[3] = (tot[3] > 0.0 ? 1.0 : 0.0) + (tot[4] > 0.0 ? 2.0 : 0.0);
        out[4] = bestf;
        out[5] = (double)bestr;
    }
}

// one workgroup per run.  col[run][kSumCol]: m, (v), min, max, bad values
__global__ __launch_bounds__(kPsumThreads) void sum_col_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, const SumRun* __restrict__ runs, int dmax,
                                                              const double* __restrict__ cols, const double* __restrict__ sys, double* __restrict__ col)
{
    __shared__ double red[kSumWaves];
    const int64_t r = blockIdx.x;
    const int y = runs[r].seg, j = runs[r].col;
    // (block_fold's order, written out: the extremes share the one pass over the tiles with the two sums)
    const int64_t t0 = tile0[y], nt = mce_seg::seg_ntiles(segs[y].n);
    const double INF = __builtin_huge_val();
    double sx = 0.0, mn = INF, mx = -INF, bad = 0.0;
    for (int64_t k = threadIdx.x; k < nt; k += kPsumThreads) {
        const double* c = cols + (t0 + k) * kSumTileCol * dmax;
        sx += c[0 * dmax + j];
        mn = c[1 * dmax + j] < mn ? c[1 * dmax + j] : mn;
        mx = c[2 * dmax + j] > mx ? c[2 * dmax + j] : mx;
        bad += c[3 * dmax + j];
    }
    sx = block_sum(sx, red);
    mn = block_min(mn, red);
    mx = block_max(mx, red);
    bad = block_sum(bad, red);
    if (threadIdx.x == 0) {
        double* out = col + r * kSumCol;
        out[0] = sx / sys[(int64_t)y * kSumSys + 0];
        out[1] = 0.0;
        out[2] = mn;
        out[3] = mx;
        out[4] = bad;
    }
}

// grid: the tiles.  part[tile][dmax]
__global__ __launch_bounds__(kPsumThreads) void sum_var_tile_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int dmax,
                                                                   const double* __restrict__ col, double* __restrict__ part)
{
    __shared__ double lds[kSumWaves][mce_sum::kSumMaxDim + 1];
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const SumSeg g = segs[s];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t ra = r0 + threadIdx.x, rb = ra + kPsumThreads;
    const double a0 = ra < r1 ? g.w[ra] : 0.0, a1 = rb < r1 ? g.w[rb] : 0.0;
    const bool u0 = mce_sum::sum_used(a0), u1 = mce_sum::sum_used(a1);
    const double* __restrict__ x0 = g.x + ra * g.ld;
    const double* __restrict__ x1 = g.x + rb * g.ld;
    for (int j = 0; j < g.d; ++j) {
        const double m = col[(g.col0 + j) * kSumCol + 0];
        double v = 0.0;
        if (u0) v = mce_sum::sum_term(a0, x0[j], m);
        if (u1) v += mce_sum::sum_term(a1, x1[j], m);
        v = wave_sum(v);
        if (lane == 0) lds[wv][j] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < g.d; j += kPsumThreads) {
        double v = lds[0][j];
        for (int k = 1; k < kSumWaves; ++k) v += lds[k][j];
        part[tile * dmax + j] = v;
    }
}

// one workgroup per run: col[run][1] = v
__global__ __launch_bounds__(kPsumThreads) void sum_var_col_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, const SumRun* __restrict__ runs,
                                                                  int dmax, const double* __restrict__ part, const double* __restrict__ sys, double* __restrict__ col)
{
    __shared__ double red[kSumWaves];
    const int64_t r = blockIdx.x;
    const int y = runs[r].seg, j = runs[r].col;
    double V;
    block_fold<1>(part + tile0[y] * dmax + j, mce_seg::seg_ntiles(segs[y].n), dmax, &V, red);
    if (threadIdx.x == 0) col[r * kSumCol + 1] = V / sys[(int64_t)y * kSumSys + 0];
}

// the run of element / scan tile `e` of a pass: the last run that begins at or below it (a run without rows shares its begin with the
// next run and is never the answer)
template <bool BY_TILE> __device__ __forceinline__ int sum_run_of(const SumRun* __restrict__ runs, int nruns, int64_t e)
{
    return mce_seg::last_at_or_below(nruns, e, [runs](int i) { return BY_TILE ? runs[i].tile0 : runs[i].begin; });
}

// grid: the elements of the pass, one thread each.  keys[e], wts[e]
__global__ __launch_bounds__(kPsumThreads) void sum_keys_kernel(const SumSeg* __restrict__ segs, const SumRun* __restrict__ runs, int nruns, int64_t total,
                                                               unsigned long long* __restrict__ keys, double* __restrict__ wts)
{
    const int64_t e = (int64_t)blockIdx.x * kPsumThreads + threadIdx.x;
    if (e >= total) return;
    const SumRun r = runs[sum_run_of<false>(runs, nruns, e)];
    const SumSeg& g = segs[r.seg];
    const int64_t i = e - r.begin;
    const double a = g.w[i];
    const bool used = mce_sum::sum_used(a);
    keys[e] = used ? mce_sum::sum_key(g.x[i * g.ld + r.col]) : mce_sum::kSumPadKey;
    wts[e] = used ? a : 0.0;
}

// grid: the scan tiles of the pass.  tot[tile]: thread t adds the elements 4 t .. 4 t + 3 of the tile in turn (an element past the
// run's end adds nothing), then block_sum
__global__ __launch_bounds__(kPsumThreads) void sum_scan_tile_kernel(const SumSeg* __restrict__ segs, const SumRun* __restrict__ runs, int nruns,
                                                                    const double* __restrict__ wts, double* __restrict__ tot)
{
    __shared__ double red[kSumWaves];
    const int64_t tile = blockIdx.x;
    const SumRun r = runs[sum_run_of<true>(runs, nruns, tile)];
    const int64_t n = segs[r.seg].n;
    const int64_t p0 = (tile - r.tile0) * kSumScanTile + 4 * (int64_t)threadIdx.x;
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (p0 + k < n) s += wts[r.begin + p0 + k];
    const double v = block_sum(s, red);
    if (threadIdx.x == 0) tot[tile] = v;
}

// grid: the runs of the pass, one wave each; lane t < nq serves target t.  quant[(first run + run) * nq + t]
__global__ __launch_bounds__(64) void sum_search_kernel(const SumSeg* __restrict__ segs, const SumRun* __restrict__ runs, int64_t run0, const double* __restrict__ q,
                                                        int nq, const double* __restrict__ sys, const unsigned long long* __restrict__ keys,
                                                        const double* __restrict__ wts, const double* __restrict__ tot, double* __restrict__ quant)
{
    const int t = threadIdx.x;
    if (t >= nq) return;
    const SumRun r = runs[blockIdx.x];
    const int64_t n = segs[r.seg].n;
    const double* s = sys + (int64_t)r.seg * kSumSys;
    const int64_t used = (int64_t)s[2];
    double* out = quant + (run0 + blockIdx.x) * nq + t;
    if (used < 1 || used > n) { *out = __builtin_nan(""); return; }
    const double target = q[t] * s[0];
    const int64_t nt = (n + kSumScanTile - 1) / kSumScanTile;
    double base = 0.0;
    int64_t k = 0;
    for (; k < nt; ++k) {
        const double next = base + tot[r.tile0 + k];
        if (next >= target) break;
        base = next;
    }
    int64_t p = used - 1;                                       // (no tile reaches the target: the last used position)
    if (k < nt) {
        const int64_t p0 = k * kSumScanTile, p1 = p0 + kSumScanTile < n ? p0 + kSumScanTile : n;
        double run;
        p = mce_sum::sum_search(wts + r.begin, p0, p1, base, target, &run);
        if (p >= p1) p = p1 - 1;                                // (the tile's tree total reached it, its running sum did not: the tile's last)
        if (p > used - 1) p = used - 1;
    }
    *out = mce_sum::sum_unkey(keys[r.begin + p]);
}

// one workgroup per system: the result block
__global__ __launch_bounds__(kPsumThreads) void sum_result_kernel(const SumSeg* __restrict__ segs, const double* __restrict__ sys, const double* __restrict__ col,
                                                                 const double* __restrict__ quant, int nq, double* __restrict__ res)
{
    __shared__ int sh_status;
    __shared__ long long sh_best;
    const int y = blockIdx.x;
    const SumSeg g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    double* out = res + g.out_off;
    if (threadIdx.x == 0) {
        int badcol = -1;
        for (int j = g.d - 1; j >= 0; --j)
            if (col[(g.col0 + j) * kSumCol + 4] > 0.0) badcol = j;
        const int flags = (int)s[3];
        int column;
        const int status = mce_sum::sum_status((flags & 1) != 0, (flags & 2) != 0, badcol, s[0], &column);
        const long long best = (long long)s[5];
        mce_sum::sum_pack_head(status, column, s[0], s[1], s[2], best, s[4], out);
        sh_status = status;
        sh_best = best;
    }
    __syncthreads();
    const bool ok = sh_status == mce_sum::kSumOk;
    const long long best = sh_best;
    const double nan = __builtin_nan("");
    double* c = out + mce_sum::kSumHead;
    for (int j = threadIdx.x; j < g.d; j += kPsumThreads) {
        const double* in = col + (g.col0 + j) * kSumCol;
        c[mce_sum::kSumMean * g.d + j] = ok ? in[0] : nan;
        c[mce_sum::kSumVar * g.d + j] = ok ? in[1] : nan;
        c[mce_sum::kSumMin * g.d + j] = ok ? mce_sum::sum_unkey(mce_sum::sum_key(in[2])) : nan;
        c[mce_sum::kSumMax * g.d + j] = ok ? mce_sum::sum_unkey(mce_sum::sum_key(in[3])) : nan;
        c[mce_sum::kSumBest * g.d + j] = (ok && best >= 0) ? g.x[best * g.ld + j] : nan;
        for (int t = 0; t < nq; ++t) c[(mce_sum::kSumPerCol + t) * g.d + j] = ok ? quant[(g.col0 + j) * nq + t] : nan;
    }
}

}  // namespace mce
