// param_marginals_kernels.hpp -- the 1-D marginal densities behind marginals= (mce_param_marginals_dev, capi_marginals.hpp) for chains
// that are already on the device.  The rule is param_marginals.hpp's; this file arranges it into launches that serve any number of
// systems (one system = one (x, ld, n, d, w) segment) by the segment-tile scheme of seg_tiles.hpp, which states the invariant these
// launches keep.  Plain C++ stores only, no atomics, 64-bit row indices.  A RUN is one (system, column).
//
//   (sum_tile / sum_sys / sum_col / sum_var_tile / sum_var_col of param_summary_kernels.hpp, as they stand: W, A2, rows, m, v, min, max)
//   mar_prep_kernel      one thread per run: the system's status, then h, c, lo, step and the column's status (prm[run][kMarPrm])
//   mar_density_kernel   the hot path.  A workgroup owns one (run, block of 256 grid points) and one PART of the system's tiles, a thread
//                        one grid point in a register.  The part's tiles are staged through LDS as (x, a) pairs, 512 rows at a time (a
//                        row that is not used as (0, 0): it adds +0.0 to a sum that is never negative), and every thread adds the
//                        staged rows in row order; all lanes read the same LDS address, which is a broadcast.  Rows whose argument is
//                        at or above 746 add +0.0 by the rule and are branched over; where that holds for a whole wave the branch is
//                        taken by the wave.  S[part][k] is written per part; the parts' boundaries depend on n alone (mar_part_tile).
//   mar_fold_kernel      per run and grid point: the parts in part order, then rho = S / ((W h) sqrt(2 pi)), into the result block
//   mar_hpd_kernel       one workgroup per run: a bitonic sort of the (rho, k) pairs in LDS on mar_before, the running sums by ONE
//                        thread in sorted order, then per probability the cut, lower, upper, pieces and edge by block reductions
//   mar_result_kernel    one workgroup per system: the head and the moment rows of the result block
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "param_marginals.hpp"
#include "param_summary_kernels.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kMarThreads = kRedThreads;
static_assert(kMarThreads == mce_mar::kMarBlock, "a thread owns one grid point of its workgroup's block");
static_assert(mce_seg::kSegTileRows == 2 * kMarThreads, "a thread stages two rows of a tile");
constexpr int kMarPrm = 8;                                      // per run: h, c, lo, step, sd, status (-1: the system failed), -, -
constexpr int kMarSysFailed = -1;

// what the marginals add to a SumSeg
struct MarSeg {
    int64_t part0;                                              // of the system's first (column, part) in S, in units of G doubles
    int64_t out_off;                                            // of the system's result block, in doubles
};

__device__ __forceinline__ double* mar_col_rows(double* block) { return block + mce_mar::kMarHead; }
__device__ __forceinline__ double* mar_p_rows(double* block, int d) { return block + mce_mar::kMarHead + (int64_t)mce_mar::kMarPerCol * d; }
__device__ __forceinline__ double* mar_dens_rows(double* block, int d, int np)
{
    return block + mce_mar::kMarHead + (int64_t)(mce_mar::kMarPerCol + mce_mar::kMarPerP * np) * d;
}

// grid: the runs, one thread each
__global__ __launch_bounds__(kMarThreads) void mar_prep_kernel(const SumSeg* __restrict__ segs, const SumRun* __restrict__ runs, int64_t nruns,
                                                              const double* __restrict__ sys, const double* __restrict__ col, int G, double scale,
                                                              double* __restrict__ prm)
{
    const int64_t r = (int64_t)blockIdx.x * kMarThreads + threadIdx.x;
    if (r >= nruns) return;
    const int y = runs[r].seg;
    const SumSeg& g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    int badcol = -1;
    for (int j = g.d - 1; j >= 0; --j)
        if (col[(g.col0 + j) * kSumCol + 4] > 0.0) badcol = j;
    int column;
    const int status = mce_mar::mar_status(((int)s[3] & 1) != 0, badcol, s[0], s[2], &column);
    double* out = prm + r * kMarPrm;
    const double nan = __builtin_nan("");
    double sd = nan, h = nan, c = nan, lo = nan, step = nan;
    int cs = kMarSysFailed;
    if (status == mce_mar::kMarOk) {
        const double* in = col + r * kSumCol;
        cs = mce_mar::mar_params(s[0], s[1], in[1], in[2], in[3], scale, G, &sd, &h, &c, &lo, &step);
    }
    out[0] = h;
    out[1] = c;
    out[2] = lo;
    out[3] = step;
    out[4] = sd;
    out[5] = (double)cs;
    out[6] = 0.0;
    out[7] = 0.0;
}

// grid: x = run * nblk + block of grid points, y = part.  S[(part0 + col * nparts + part) * G + k]
__global__ __launch_bounds__(kMarThreads) void mar_density_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const SumRun* __restrict__ runs,
                                                                 const double* __restrict__ prm, int G, int nblk, double* __restrict__ S)
{
    __shared__ double2 stage[mce_seg::kSegTileRows];
    const int64_t r = blockIdx.x / nblk;
    const int blk = blockIdx.x % nblk, part = blockIdx.y;
    const int y = runs[r].seg, j = runs[r].col;
    const SumSeg g = segs[y];
    const int nparts = mce_mar::mar_nparts(g.n);
    if (part >= nparts) return;                                  // (a launch is sized by the call's largest part count)
    const double* p = prm + r * kMarPrm;
    if ((int)p[5] != mce_mar::kMarOk) return;
    const double c = p[1];
    const int k = blk * kMarThreads + threadIdx.x;
    const bool mine = k < G;
    const double gk = mce_mar::mar_grid_point(p[2], p[3], mine ? k : 0);
    const int64_t t0 = mce_mar::mar_part_tile(g.n, part), t1 = mce_mar::mar_part_tile(g.n, part + 1);
    double acc = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t r0 = t * mce_seg::kSegTileRows;
        const int64_t left = g.n - r0;
        const int cnt = left < mce_seg::kSegTileRows ? (int)left : mce_seg::kSegTileRows;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int at = threadIdx.x + q * kMarThreads;
            if (at < cnt) {
                const int64_t i = r0 + at;
                const double a = g.w[i];
                const bool used = mce_sum::sum_used(a);
                stage[at] = make_double2(used ? g.x[i * g.ld + j] : 0.0, used ? a : 0.0);
            }
        }
        __syncthreads();
        if (mine) {
            for (int i = 0; i < cnt; ++i) {
                const double2 xa = stage[i];
                const double arg = mce_mar::mar_arg(c, gk, xa.x);
                if (arg < mce_kde::kKdeUnderflow) acc = mce_mar::mar_add(acc, xa.y, arg);
            }
        }
    }
    if (mine) S[(msegs[y].part0 + (int64_t)j * nparts + part) * G + k] = acc;
}

// grid: run * nblk + block of grid points.  The densities go to the system's result block.
__global__ __launch_bounds__(kMarThreads) void mar_fold_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const SumRun* __restrict__ runs,
                                                              const double* __restrict__ prm, const double* __restrict__ sys, int G, int nblk, int np,
                                                              const double* __restrict__ S, double* __restrict__ res)
{
    const int64_t r = blockIdx.x / nblk;
    const int k = (int)(blockIdx.x % nblk) * kMarThreads + threadIdx.x;
    if (k >= G) return;
    const int y = runs[r].seg, j = runs[r].col;
    const SumSeg& g = segs[y];
    const double* p = prm + r * kMarPrm;
    double rho = __builtin_nan("");
    if ((int)p[5] == mce_mar::kMarOk) {
        const int nparts = mce_mar::mar_nparts(g.n);
        const double* src = S + (msegs[y].part0 + (int64_t)j * nparts) * G + k;
        double acc = 0.0;
        for (int q = 0; q < nparts; ++q) acc += src[(int64_t)q * G];
        rho = acc / mce_mar::mar_norm(sys[(int64_t)y * kSumSys + 0], p[0]);
    }
    mar_dens_rows(res + msegs[y].out_off, g.d, np)[(int64_t)j * G + k] = rho;
}

// grid: the runs, one workgroup each
__global__ __launch_bounds__(kMarThreads) void mar_hpd_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const SumRun* __restrict__ runs,
                                                             const double* __restrict__ prm, const double* __restrict__ probs, int np, int G,
                                                             double* __restrict__ res)
{
    __shared__ double s_rho[mce_mar::kMarMaxGrid];
    __shared__ double s_cum[mce_mar::kMarMaxGrid];
    __shared__ int s_k[mce_mar::kMarMaxGrid];
    __shared__ unsigned char s_sel[mce_mar::kMarMaxGrid];
    __shared__ double red[kRedWaves];
    const int64_t r = blockIdx.x;
    const int y = runs[r].seg, j = runs[r].col;
    const int d = segs[y].d;
    double* block = res + msegs[y].out_off;
    double* colr = mar_col_rows(block);
    double* pr = mar_p_rows(block, d);
    const double* p = prm + r * kMarPrm;
    const int cs = (int)p[5];
    const double nan = __builtin_nan("");
    if (cs != mce_mar::kMarOk) {
        if (threadIdx.x == 0) {
            colr[mce_mar::kMarMode * d + j] = nan;
            colr[mce_mar::kMarModeDensity * d + j] = nan;
            for (int t = 0; t < np; ++t) {
                double* o = pr + (int64_t)t * mce_mar::kMarPerP * d + j;
                o[mce_mar::kMarLower * d] = nan;
                o[mce_mar::kMarUpper * d] = nan;
                o[mce_mar::kMarPieces * d] = cs == kMarSysFailed ? nan : -1.0;
                o[mce_mar::kMarEdge * d] = nan;
            }
        }
        return;
    }
    const double lo = p[2], step = p[3];
    const double* rho = mar_dens_rows(block, d, np) + (int64_t)j * G;
    for (int k = threadIdx.x; k < G; k += kMarThreads) { s_rho[k] = rho[k]; s_k[k] = k; }
    __syncthreads();
    // the bitonic network on mar_before: G is a power of two
    for (int size = 2; size <= G; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int a = threadIdx.x; a < G; a += kMarThreads) {
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
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int q = 0; q < G; ++q) { run += s_rho[q]; s_cum[q] = run; }
        colr[mce_mar::kMarMode * d + j] = mce_mar::mar_grid_point(lo, step, s_k[0]);
        colr[mce_mar::kMarModeDensity * d + j] = s_rho[0];
    }
    __syncthreads();
    const double Z = s_cum[G - 1];
    for (int t = 0; t < np; ++t) {
        const double target = probs[t] * Z;
        double first = (double)(G - 1);                          // (no position reaches the target: all of them)
        for (int q = threadIdx.x; q < G; q += kMarThreads)
            if (s_cum[q] >= target && (double)q < first) first = (double)q;
        const int cut = (int)block_min(first, red);
        __syncthreads();
        for (int q = threadIdx.x; q < G; q += kMarThreads) s_sel[s_k[q]] = q <= cut ? 1 : 0;
        __syncthreads();
        double kmin = (double)G, kmax = -1.0, pieces = 0.0;
        for (int k = threadIdx.x; k < G; k += kMarThreads) {
            if (!s_sel[k]) continue;
            kmin = (double)k < kmin ? (double)k : kmin;
            kmax = (double)k > kmax ? (double)k : kmax;
            pieces += (k == 0 || !s_sel[k - 1]) ? 1.0 : 0.0;
        }
        kmin = block_min(kmin, red);
        kmax = block_max(kmax, red);
        pieces = block_sum(pieces, red);
        if (threadIdx.x == 0) {
            double* o = pr + (int64_t)t * mce_mar::kMarPerP * d + j;
            o[mce_mar::kMarLower * d] = mce_mar::mar_grid_point(lo, step, (int)kmin);
            o[mce_mar::kMarUpper * d] = mce_mar::mar_grid_point(lo, step, (int)kmax);
            o[mce_mar::kMarPieces * d] = pieces;
            o[mce_mar::kMarEdge * d] = (s_sel[0] || s_sel[G - 1]) ? 1.0 : 0.0;
        }
        __syncthreads();
    }
}

// one workgroup per system: the head and the moment rows
__global__ __launch_bounds__(kMarThreads) void mar_result_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const double* __restrict__ sys,
                                                                const double* __restrict__ col, const double* __restrict__ prm, int G, int np,
                                                                double* __restrict__ res)
{
    const int y = blockIdx.x;
    const SumSeg g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    double* out = res + msegs[y].out_off;
    if (threadIdx.x == 0) {
        int badcol = -1;
        for (int j = g.d - 1; j >= 0; --j)
            if (col[(g.col0 + j) * kSumCol + 4] > 0.0) badcol = j;
        int column;
        const int status = mce_mar::mar_status(((int)s[3] & 1) != 0, badcol, s[0], s[2], &column);
        mce_mar::mar_pack_head(status, column, s[0], s[1], s[2], G, np, out);
    }
    const double nan = __builtin_nan("");
    double* c = mar_col_rows(out);
    for (int j = threadIdx.x; j < g.d; j += kMarThreads) {
        const double* in = col + (g.col0 + j) * kSumCol;
        const double* p = prm + (g.col0 + j) * kMarPrm;
        const int cs = (int)p[5];
        const bool ok = cs == mce_mar::kMarOk;
        c[mce_mar::kMarMean * g.d + j] = ok ? in[0] : nan;
        c[mce_mar::kMarVar * g.d + j] = ok ? in[1] : nan;
        c[mce_mar::kMarSd * g.d + j] = ok ? p[4] : nan;
        c[mce_mar::kMarH * g.d + j] = ok ? p[0] : nan;
        c[mce_mar::kMarC * g.d + j] = ok ? p[1] : nan;
        c[mce_mar::kMarLo * g.d + j] = ok ? p[2] : nan;
        c[mce_mar::kMarStep * g.d + j] = ok ? p[3] : nan;
        c[mce_mar::kMarColStatus * g.d + j] = cs == kMarSysFailed ? nan : (double)cs;
    }
}

}  // namespace mce
