// param_marginals_kernels.hpp -- the 1-D marginal densities behind marginals= (mce_param_marginals_dev and, with bounds=,
// mce_param_marginals_bounded_dev: capi_marginals.hpp) for chains that are already on the device.  The rules are param_marginals.hpp's and
// param_marginals_bounds.hpp's; this file arranges them into launches that serve any number of systems (one system = one (x, ld, n, d,
// w) segment) by the segment-tile scheme of seg_tiles.hpp, which states the invariant these launches keep.  Plain C++ stores only, no
// atomics, 64-bit row indices.  A RUN is one (system, column).
//
// Every kernel is ONE template on kBounds: <false> is the rule without bounds, <true> the rule with them, and what differs between the
// two is MarForm<kBounds> or an `if constexpr`.  The <false> instances hold nothing of the bounded rule: one sum, no bounds reads.
//
//   (sum_tile / sum_sys / sum_col / sum_var_tile / sum_var_col of param_summary_kernels.hpp, as they stand: W, A2, rows, m, v, min, max)
//   mar_prep_kernel      one thread per run: the system's status (mar_sys_status, which con_prep and con_result call too), then h, c, lo,
//                        step and the column's status (prm[run][MarForm::kPrm]);
//                        <true>: step 3' from bnd[run][2] = L, U, and L, U, at_lo, at_hi behind them
//   mar_density_kernel   the hot path.  A workgroup owns one (run, block of 256 grid points) and one PART of the system's tiles, a thread
//                        one grid point in a register.  The part's tiles are staged through LDS as (x, a) pairs, 512 rows at a time (a
//                        row that is not used as (0, 0): it adds +0.0 to a sum that is never negative), and every thread adds the
//                        staged rows in row order; all lanes read the same LDS address, which is a broadcast.  Rows whose argument is
//                        at or above 746 add +0.0 by the rule and are branched over; where that holds for a whole wave the branch is
//                        taken by the wave.  <false>: S[part][k] is written per part.  <true>: TWO sums, S += t and R += t (x - g),
//                        t = a exp(-arg) formed once, at S[part][{0, 1}][k].  The parts' boundaries depend on n alone (mar_part_tile).
//   mar_fold_kernel      per run and grid point: the parts in part order, then rho = S / ((W h) sqrt(2 pi)) (<true>: both sums, then
//                        steps 5' and 6'), into the result block
//   mar_hpd_kernel       one workgroup per run: density_order.hpp's sort of the (rho, k) pairs in LDS, the running sums by ONE thread in
//                        sorted order (<true>: with the end weights of step 8'), then per probability the cut, lower, upper, pieces and
//                        edge by block reductions
//   mar_result_kernel    one workgroup per system: the head and the per-column rows of the result block
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "density_order.hpp"
#include "param_marginals.hpp"
#include "param_marginals_bounds.hpp"
#include "param_summary_kernels.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kMarThreads = kRedThreads;
static_assert(kMarThreads == mce_mar::kMarBlock, "a thread owns one grid point of its workgroup's block");
static_assert(mce_seg::kSegTileRows == 2 * kMarThreads, "a thread stages two rows of a tile");
constexpr int kMarSysFailed = -1;

// what the two rules lay out differently
template <bool kBounds> struct MarForm {
    // per run: h, c, lo, step, sd, status (-1: the system failed), -, -; with bounds then L, U, at_lo, at_hi
    static constexpr int kPrm = kBounds ? 12 : 8;
    static constexpr int kPerCol = kBounds ? mce_marb::kMarbPerCol : mce_mar::kMarPerCol;      // per-column rows of a result block
    static constexpr int kSums = kBounds ? 2 : 1;               // sums per part and grid point: S; with bounds S, then R
};

// what the marginals add to a SumSeg
struct MarSeg {
    int64_t part0;                                              // of the system's first (column, part) in S, in units of kSums * G doubles
    int64_t out_off;                                            // of the system's result block, in doubles
};

__device__ __forceinline__ double* mar_col_rows(double* block) { return block + mce_mar::kMarHead; }
template <bool kBounds> __device__ __forceinline__ double* mar_p_rows(double* block, int d)
{
    return block + mce_mar::kMarHead + (int64_t)MarForm<kBounds>::kPerCol * d;
}
template <bool kBounds> __device__ __forceinline__ double* mar_dens_rows(double* block, int d, int np)
{
    return block + mce_mar::kMarHead + (int64_t)(MarForm<kBounds>::kPerCol + mce_mar::kMarPerP * np) * d;
}

// the system's status from the moment kernels' outputs (s: its kSumSys sums; all d columns of the segment count: the lowest refused one)
__device__ __forceinline__ int mar_sys_status(const SumSeg& g, const double* __restrict__ s, const double* __restrict__ col, int* column)
{
    int badcol = -1;
    for (int j = g.d - 1; j >= 0; --j)
        if (col[(g.col0 + j) * kSumCol + 4] > 0.0) badcol = j;
    return mce_mar::mar_status(((int)s[3] & 1) != 0, badcol, s[0], s[2], column);
}

// grid: the runs, one thread each.  bnd[run][2]: L, U (<false>: not read)
template <bool kBounds>
__global__ __launch_bounds__(kMarThreads) void mar_prep_kernel(const SumSeg* __restrict__ segs, const SumRun* __restrict__ runs, int64_t nruns,
                                                              const double* __restrict__ sys, const double* __restrict__ col, const double* __restrict__ bnd,
                                                              int G, double scale, double* __restrict__ prm)
{
    const int64_t r = (int64_t)blockIdx.x * kMarThreads + threadIdx.x;
    if (r >= nruns) return;
    const int y = runs[r].seg;
    const SumSeg& g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    int column;
    const int status = mar_sys_status(g, s, col, &column);
    double* out = prm + r * MarForm<kBounds>::kPrm;
    const double nan = __builtin_nan("");
    double sd = nan, h = nan, c = nan, lo = nan, step = nan;
    int cs = kMarSysFailed;
    const double* in = col + r * kSumCol;
    if constexpr (kBounds) {
        const double L = bnd[2 * r], U = bnd[2 * r + 1];
        double at_lo = nan, at_hi = nan;
        if (status == mce_mar::kMarOk) cs = mce_marb::marb_params(s[0], s[1], in[1], in[2], in[3], L, U, scale, G, &sd, &h, &c, &lo, &step, &at_lo, &at_hi);
        out[8] = L;
        out[9] = U;
        out[10] = at_lo;
        out[11] = at_hi;
    } else {
        if (status == mce_mar::kMarOk) cs = mce_mar::mar_params(s[0], s[1], in[1], in[2], in[3], scale, G, &sd, &h, &c, &lo, &step);
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

// grid: x = run * nblk + block of grid points, y = part.  S[((part0 + col * nparts + part) * kSums + {0: S, 1: R}) * G + k]
template <bool kBounds>
__global__ __launch_bounds__(kMarThreads) void mar_density_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const SumRun* __restrict__ runs,
                                                                 const double* __restrict__ prm, int G, int nblk, double* __restrict__ S)
{
    using F = MarForm<kBounds>;
    __shared__ double2 stage[mce_seg::kSegTileRows];
    const int64_t r = blockIdx.x / nblk;
    const int blk = blockIdx.x % nblk, part = blockIdx.y;
    const int y = runs[r].seg, j = runs[r].col;
    const SumSeg g = segs[y];
    const int nparts = mce_mar::mar_nparts(g.n);
    if (part >= nparts) return;                                  // (a launch is sized by the call's largest part count)
    const double* p = prm + r * F::kPrm;
    if ((int)p[5] != mce_mar::kMarOk) return;
    const double c = p[1];
    const int k = blk * kMarThreads + threadIdx.x;
    const bool mine = k < G;
    const double gk = mce_mar::mar_grid_point(p[2], p[3], mine ? k : 0);
    const int64_t t0 = mce_mar::mar_part_tile(g.n, part), t1 = mce_mar::mar_part_tile(g.n, part + 1);
    double acc = 0.0;
    [[maybe_unused]] double R = 0.0;                             // (with bounds alone)
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
                if constexpr (kBounds) {
                    mce_marb::marb_term(c, gk, xa.x, xa.y, &acc, &R);
                } else {
                    const double arg = mce_mar::mar_arg(c, gk, xa.x);
                    if (arg < mce_kde::kKdeUnderflow) acc = mce_mar::mar_add(acc, xa.y, arg);
                }
            }
        }
    }
    if (mine) {
        double* dst = S + (msegs[y].part0 + (int64_t)j * nparts + part) * F::kSums * G + k;
        dst[0] = acc;
        if constexpr (kBounds) dst[G] = R;
    }
}

// grid: run * nblk + block of grid points.  The densities go to the system's result block.
template <bool kBounds>
__global__ __launch_bounds__(kMarThreads) void mar_fold_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const SumRun* __restrict__ runs,
                                                              const double* __restrict__ prm, const double* __restrict__ sys, int G, int nblk, int np,
                                                              const double* __restrict__ S, double* __restrict__ res)
{
    using F = MarForm<kBounds>;
    const int64_t r = blockIdx.x / nblk;
    const int k = (int)(blockIdx.x % nblk) * kMarThreads + threadIdx.x;
    if (k >= G) return;
    const int y = runs[r].seg, j = runs[r].col;
    const SumSeg& g = segs[y];
    const double* p = prm + r * F::kPrm;
    double rho = __builtin_nan("");
    if ((int)p[5] == mce_mar::kMarOk) {
        const int nparts = mce_mar::mar_nparts(g.n);
        const double* src = S + (msegs[y].part0 + (int64_t)j * nparts) * F::kSums * G + k;
        double acc = 0.0;
        [[maybe_unused]] double R = 0.0;
        for (int q = 0; q < nparts; ++q) {
            acc += src[(int64_t)q * F::kSums * G];
            if constexpr (kBounds) R += src[(int64_t)q * F::kSums * G + G];
        }
        const double h = p[0];
        const double norm = mce_mar::mar_norm(sys[(int64_t)y * kSumSys + 0], h);
        if constexpr (kBounds) {
            double a0, a1, a2, den;
            mce_marb::marb_consts(mce_mar::mar_grid_point(p[2], p[3], k), p[8], p[9], h, &a0, &a1, &a2, &den);
            rho = mce_marb::marb_density(mce_marb::marb_t0(acc, norm), mce_marb::marb_t1(R, h, norm), a0, a1, a2, den);
        } else {
            rho = acc / norm;
        }
    }
    mar_dens_rows<kBounds>(res + msegs[y].out_off, g.d, np)[(int64_t)j * G + k] = rho;
}

// grid: the runs, one workgroup each
template <bool kBounds>
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
    double* pr = mar_p_rows<kBounds>(block, d);
    const double* p = prm + r * MarForm<kBounds>::kPrm;
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
    const double* rho = mar_dens_rows<kBounds>(block, d, np) + (int64_t)j * G;
    for (int k = threadIdx.x; k < G; k += kMarThreads) { s_rho[k] = rho[k]; s_k[k] = k; }
    __syncthreads();
    order_sort(s_rho, s_k, G);                                   // (G is a power of two)
    if (threadIdx.x == 0) {
        if constexpr (kBounds) {
            const bool at_lo = p[10] != 0.0, at_hi = p[11] != 0.0;
            order_running_sum(s_rho, s_k, G, s_cum, [=](double v, int k) { return mce_marb::marb_weighted(v, k, G, at_lo, at_hi); });
        } else {
            order_running_sum(s_rho, G, s_cum);
        }
        colr[mce_mar::kMarMode * d + j] = mce_mar::mar_grid_point(lo, step, s_k[0]);
        colr[mce_mar::kMarModeDensity * d + j] = s_rho[0];
    }
    __syncthreads();
    const double Z = s_cum[G - 1];
    for (int t = 0; t < np; ++t) {
        const int cut = order_cut(s_cum, G, probs[t] * Z, red);
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

// one workgroup per system: the head and the per-column rows (<true>: the head's reserved slot holds 1, and the bounds' rows)
template <bool kBounds>
__global__ __launch_bounds__(kMarThreads) void mar_result_kernel(const SumSeg* __restrict__ segs, const MarSeg* __restrict__ msegs, const double* __restrict__ sys,
                                                                const double* __restrict__ col, const double* __restrict__ prm, int G, int np,
                                                                double* __restrict__ res)
{
    const int y = blockIdx.x;
    const SumSeg g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    double* out = res + msegs[y].out_off;
    if (threadIdx.x == 0) {
        int column;
        const int status = mar_sys_status(g, s, col, &column);
        mce_mar::mar_pack_head(status, column, s[0], s[1], s[2], G, np, out);
        if constexpr (kBounds) out[mce_mar::kMarReserved] = 1.0;
    }
    const double nan = __builtin_nan("");
    double* c = mar_col_rows(out);
    for (int j = threadIdx.x; j < g.d; j += kMarThreads) {
        const double* in = col + (g.col0 + j) * kSumCol;
        const double* p = prm + (g.col0 + j) * MarForm<kBounds>::kPrm;
        const int cs = (int)p[5];
        const bool ok = cs == mce_mar::kMarOk, sys_ok = cs != kMarSysFailed;
        c[mce_mar::kMarMean * g.d + j] = ok ? in[0] : nan;
        c[mce_mar::kMarVar * g.d + j] = ok ? in[1] : nan;
        c[mce_mar::kMarSd * g.d + j] = ok ? p[4] : nan;
        c[mce_mar::kMarH * g.d + j] = ok ? p[0] : nan;
        c[mce_mar::kMarC * g.d + j] = ok ? p[1] : nan;
        c[mce_mar::kMarLo * g.d + j] = ok ? p[2] : nan;
        c[mce_mar::kMarStep * g.d + j] = ok ? p[3] : nan;
        c[mce_mar::kMarColStatus * g.d + j] = sys_ok ? (double)cs : nan;
        if constexpr (kBounds) {
            c[mce_marb::kMarbBoundLo * g.d + j] = sys_ok ? p[8] : nan;
            c[mce_marb::kMarbBoundHi * g.d + j] = sys_ok ? p[9] : nan;
            c[mce_marb::kMarbAtLo * g.d + j] = ok ? p[10] : nan;
            c[mce_marb::kMarbAtHi * g.d + j] = ok ? p[11] : nan;
        }
    }
}

}  // namespace mce
