// param_contours_kernels.hpp -- the 2-D joint densities behind contours= (mce_param_contours_dev, capi_contours.hpp) for chains that are
// already on the device.  The rule is param_contours.hpp's; this file arranges it into launches that serve any number of systems (one
// system = one (x, ld, n, d, w) segment) by the segment-tile scheme of seg_tiles.hpp, which states the invariant these launches keep.
// Plain C++ stores only, no atomics, 64-bit row indices.  cols[nc] (the chosen columns) is one list per call.
//
//   (sum_tile / sum_sys / sum_col / sum_var_tile / sum_var_col of param_summary_kernels.hpp, as they stand: W, A2, rows, m, v, min, max)
//   con_prep_kernel      one thread per (system, chosen column): the system's status (mar_sys_status of param_marginals_kernels.hpp),
//                        then h, c, lo, step and the column's status
//   con_density_kernel   the hot path.  A workgroup of four waves owns one x column, a GROUP of up to kConJB partner columns and one PART of
//                        the system's tiles.  Per chunk of 16 rows it stages (x, a) of its columns, forms the (1 + kConJB) * 16 * G kernel
//                        values into LDS (the x column's already times the weight; a row that is not used, or past the end, as zeros), and
//                        runs four k-steps of v_mfma_f64_16x16x4_f64 on every 16 x 16 block of cells the wave owns:
//                        A = a_r E_i[r][16 bi + (lane & 15)], B = E_j[r][16 bj + (lane & 15)], r = 4 ks + (lane >> 4).  Every block's chain
//                        visits the part's rows in row order, so a pair's bits depend on the system's rows, the two columns, G and scale
//                        alone.  S[part][pair][G * G] is written per part; the parts' boundaries depend on n alone (con_part_tile).
//   con_fold_kernel      per (system, pair) and block of 256 cells: the parts in part order, then rho = S / (W h_i h_j 2 pi), into the block
//   con_region_kernel    one workgroup per (system, pair): density_order.hpp's sort of the (rho, k) pairs in LDS, the running sums by
//                        ONE thread in sorted order, then per probability the cut by all threads, box and edge by block reductions
//   con_result_kernel    one workgroup per system: the head and the column rows of the result block
//
// Every kernel is ONE text with a bool template parameter: <false> is the rule without bounds, <true> the rule with hard prior bounds
// (mce_param_contours_bounded_dev; steps 3" .. 8" of param_contours.hpp).  What <true> adds: con_prep_kernel forms the grid that ends on a
// bound, status 8 and the table of a0, a1, a2, den per (system, chosen column, grid point); con_density_kernel stages a second value per
// (row, grid point) of a column that is not open -- (a E_x) (x - g) of the x column, E_y (y - g) of a partner -- and runs two more MFMA
// chains per block, R_x += A' B and R_y += A B', each skipped wave-uniformly where its column is open; con_fold_kernel folds the three
// sums in part order and applies step 6"; con_region_kernel weighs the running sum; con_result_kernel writes the bounds' rows.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "density_order.hpp"
#include "param_contours.hpp"
#include "param_marginals_kernels.hpp"
#include "param_summary_kernels.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kConThreads = kRedThreads;
constexpr int kConWaves = kRedWaves;
static_assert(kConThreads == mce_con::kConBlock, "a fold thread owns one cell of its workgroup's block");
constexpr int kConSysFailed = -1;
#ifndef MCE_CON_JB
#define MCE_CON_JB 2                                            // (docs/design/contours.md has 1, 2, 3, 4 and 8 timed)
#endif
constexpr int kConJB = MCE_CON_JB;                              // partner columns of a group
#ifndef MCE_CONB_JB
#define MCE_CONB_JB 1                                           // (docs/design/contours_bounds.md has 1 and 2 timed: 1 is faster)
#endif
// what the two rules lay out differently
template <bool kBounds> struct ConForm {
    // per (system, chosen column): h, c, lo, step, sd, status (-1: the system failed), -, -; with bounds then L, U, at_lo, at_hi
    static constexpr int kPrm = kBounds ? 12 : 8;
    static constexpr int kPerCol = kBounds ? mce_con::kConbPerCol : mce_con::kConPerCol;       // per-column rows of a result block
    static constexpr int kSums = kBounds ? 3 : 1;               // sums per part, pair and cell: S; with bounds S, then R_x, then R_y
    static constexpr int kJB = kBounds ? MCE_CONB_JB : kConJB;  // partner columns of a group
    static constexpr int kVals = kBounds ? 2 : 1;               // staged values per (slot, row, grid point): E; with bounds then E (x - g)
};
constexpr int kConTab = 4;                                      // per (system, chosen column, grid point): a0, a1, a2, den
constexpr int kConChunkRows = 16;                               // rows staged at a time: four k-steps of four rows
static_assert(mce_seg::kSegTileRows % kConChunkRows == 0, "a tile is whole chunks");

typedef double con_v4d __attribute__((ext_vector_type(4)));

// what the contours add to a SumSeg
struct ConSeg {
    int64_t part0;                                              // of the system's first part in S, in units of P * G * G doubles
    int64_t out_off;                                            // of the system's result block, in doubles
};
// one group of a call: the x column cols[s] with the partners cols[t0 .. t0 + cnt)
struct ConGroup {
    int32_t s, t0, cnt, pair0;                                  // pair0: the pair (s, t0); the group's pairs are consecutive
};

__device__ __forceinline__ double* con_col_rows(double* block) { return block + mce_con::kConHead; }
template <bool kBounds> __device__ __forceinline__ double* con_pair_rows(double* block, int nc)
{
    return block + mce_con::kConHead + (int64_t)ConForm<kBounds>::kPerCol * nc;
}
template <bool kBounds> __device__ __forceinline__ double* con_p_rows(double* block, int nc)
{
    return con_pair_rows<kBounds>(block, nc) + (int64_t)mce_con::kConPerPair * mce_con::con_npairs(nc);
}
template <bool kBounds> __device__ __forceinline__ double* con_dens_rows(double* block, int nc, int np)
{
    return con_p_rows<kBounds>(block, nc) + (int64_t)mce_con::kConPerP * np * mce_con::con_npairs(nc);
}

// grid: the (system, chosen column) pairs, one thread each.  prm[(system * nc + t)][kPrm].  <true>: bnd[system][2 * nc] = lo[nc], hi[nc];
// tab[(system * nc + t) * G + k][kConTab] = step 5' at the grid point k (erf once per column and grid point, not once per cell)
template <bool kBounds>
__global__ __launch_bounds__(kConThreads) void con_prep_kernel(const SumSeg* __restrict__ segs, int nseg, const int32_t* __restrict__ cols, int nc,
                                                              const double* __restrict__ sys, const double* __restrict__ col, const double* __restrict__ bnd, int G,
                                                              double scale, double* __restrict__ prm, double* __restrict__ tab)
{
    const int64_t r = (int64_t)blockIdx.x * kConThreads + threadIdx.x;
    if (r >= (int64_t)nseg * nc) return;
    const int y = (int)(r / nc), t = (int)(r % nc);
    const SumSeg& g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    int column;
    const int status = mar_sys_status(g, s, col, &column);
    double* out = prm + r * ConForm<kBounds>::kPrm;
    const double nan = __builtin_nan("");
    double sd = nan, h = nan, c = nan, lo = nan, step = nan;
    int cs = kConSysFailed;
    const double* in = col + (g.col0 + cols[t]) * kSumCol;
    if constexpr (kBounds) {
        const double L = bnd[(int64_t)y * 2 * nc + t], U = bnd[(int64_t)y * 2 * nc + nc + t];
        double at_lo = nan, at_hi = nan;
        if (status == mce_mar::kMarOk) cs = mce_con::conb_params(s[0], s[1], in[1], in[2], in[3], L, U, scale, G, &sd, &h, &c, &lo, &step, &at_lo, &at_hi);
        out[8] = L;
        out[9] = U;
        out[10] = at_lo;
        out[11] = at_hi;
        if (cs == mce_con::kConOk) {
            double* q = tab + r * G * kConTab;
            for (int k = 0; k < G; ++k, q += kConTab) mce_marb::marb_consts(mce_mar::mar_grid_point(lo, step, k), L, U, h, q, q + 1, q + 2, q + 3);
        }
    } else {
        if (status == mce_mar::kMarOk) cs = mce_con::con_params(s[0], s[1], in[1], in[2], in[3], scale, G, &sd, &h, &c, &lo, &step);
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

// grid: x = system * ngroups + group, y = part.  S[(((part0 + part) * P + pair) * kSums + {0: S, 1: R_x, 2: R_y}) * G * G + kx * G + ky]; the R of a
// column that is open on both sides is not written (the fold takes it as +0.0).
// LDS (dynamic, ConTile<G, kBounds>::kLdsBytes): E[kVals][1 + kJB][16][G + 16]: plane 0, slot 0 the x column's a_r E_i[r][k], slot 1 + q partner q's
// E_j[r][k]; <true>: plane 1 the same times x - g, formed for a slot whose column is not open.  The row stride G + 16 is = 16 mod 32 doubles, so a
// fragment read hits each bank once (cov_gram_kernel's comment).  Wave wv owns the block row bi = wv % (G / 16) of every pair of the group and
// kNbj block columns from bj0 = (wv / (G / 16)) * kNbj: at G = 64 all four, at G = 32 one.
template <int G, bool kBounds = false> struct ConTile {
    static constexpr int kJB = ConForm<kBounds>::kJB;
    static constexpr int kNb = G / 16;                          // blocks of 16 cells along an axis
    static constexpr int kNbj = kNb * kNb / kConWaves;          // block columns of a wave: 4 at G = 64, 1 at G = 32
    static constexpr int kStride = G + 16;
    static constexpr int kValues = (1 + kJB) * kConChunkRows * G;
    static constexpr int kPlane = (1 + kJB) * kConChunkRows * kStride;                                        // doubles of a plane of E
    static constexpr size_t kLdsBytes = (size_t)ConForm<kBounds>::kVals * kPlane * sizeof(double);            // dynamic: E
    static_assert(kNbj >= 1 && kNb * kNb == kNbj * kConWaves && kStride % 32 == 16 && kValues % kConThreads == 0, "the wave's share of a pair");
    static_assert((1 + kJB) * kConChunkRows <= kConThreads, "a staging thread per (slot, row)");
};

template <int G, bool kBounds>
__global__ __launch_bounds__(kConThreads) void con_density_kernel(const SumSeg* __restrict__ segs, const ConSeg* __restrict__ csegs, const ConGroup* __restrict__ groups,
                                                                 int ngroups, const int32_t* __restrict__ cols, int nc, const double* __restrict__ prm,
                                                                 double* __restrict__ S)
{
    using T = ConTile<G, kBounds>;
    constexpr int kJB = T::kJB, kPrm = ConForm<kBounds>::kPrm, kSums = ConForm<kBounds>::kSums;
    extern __shared__ double con_E[];                            // [kVals][(1 + kJB) * kConChunkRows][T::kStride]: T::kLdsBytes
    double* E = con_E;
    __shared__ double xs[(1 + kJB) * kConChunkRows];
    __shared__ double as[kConChunkRows];
    __shared__ double pc[1 + kJB], plo[1 + kJB], pstep[1 + kJB];
    __shared__ int pmom[1 + kJB];                                // <true>: the slot's column is not open: its second value is formed
    const int y = blockIdx.x / ngroups, part = blockIdx.y;
    const ConGroup grp = groups[blockIdx.x - y * ngroups];
    const SumSeg g = segs[y];
    const int nparts = mce_con::con_nparts(g.n);
    if (part >= nparts) return;                                  // (a launch is sized by the call's largest part count)
    const double* px = prm + ((int64_t)y * nc + grp.s) * kPrm;
    if ((int)px[5] != mce_con::kConOk) return;                   // (the system failed, or the x column did: the fold writes NaN)
    if (threadIdx.x < 1 + kJB) {
        // a slot past the group's end repeats the x column: its values are formed and never used
        const bool live = threadIdx.x == 0 || threadIdx.x - 1 < grp.cnt;
        const int t = threadIdx.x == 0 ? grp.s : (live ? grp.t0 + threadIdx.x - 1 : grp.s);
        const double* p = prm + ((int64_t)y * nc + t) * kPrm;
        pc[threadIdx.x] = p[1];
        plo[threadIdx.x] = p[2];
        pstep[threadIdx.x] = p[3];
        if constexpr (kBounds) pmom[threadIdx.x] = (live && !mce_con::conb_open(p[8], p[9])) ? 1 : 0;
    }
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int bi = wv % T::kNb, bj0 = (wv / T::kNb) * T::kNbj;
    const int frow = lane >> 4, fcol = lane & 15;
    con_v4d acc[kSums][kJB][T::kNbj];
#pragma unroll
    for (int z = 0; z < kSums; ++z)
#pragma unroll
        for (int q = 0; q < kJB; ++q)
#pragma unroll
            for (int b = 0; b < T::kNbj; ++b) acc[z][q][b] = con_v4d{0.0, 0.0, 0.0, 0.0};
    const int64_t row0 = mce_con::con_part_tile(g.n, part) * mce_seg::kSegTileRows;
    const int64_t rend = mce_con::con_part_tile(g.n, part + 1) * mce_seg::kSegTileRows;
    const int64_t row1 = rend < g.n ? rend : g.n;
    // the staging thread's slot and row
    const int sslot = threadIdx.x / kConChunkRows, srow = threadIdx.x % kConChunkRows;
    const int scol = sslot == 0 ? cols[grp.s] : (sslot - 1 < grp.cnt ? cols[grp.t0 + sslot - 1] : cols[grp.s]);
    for (int64_t c0 = row0; c0 < row1; c0 += kConChunkRows) {
        __syncthreads();                                        // (the parameters are written; the last chunk's values are read)
        if (sslot < 1 + kJB) {
            const int64_t r = c0 + srow;
            const double a = r < row1 ? g.w[r] : 0.0;
            const bool used = mce_sum::sum_used(a);
            xs[sslot * kConChunkRows + srow] = used ? g.x[r * g.ld + scol] : 0.0;
            if (sslot == 0) as[srow] = used ? a : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int v = threadIdx.x; v < T::kValues; v += kConThreads) {
            const int k = v % G, row = (v / G) % kConChunkRows, slot = v / (G * kConChunkRows);
            const double a = as[row];
            double e = 0.0, m = 0.0;
            if (a != 0.0) {                                      // (a row that is not used is staged as zeros: its x may be anything)
                const double gk = mce_mar::mar_grid_point(plo[slot], pstep[slot], k), xv = xs[slot * kConChunkRows + row];
                e = mce_con::con_value(pc[slot], gk, xv);
                if (slot == 0) e = mce_con::con_weighted(a, e);
                if constexpr (kBounds) m = mce_con::conb_moment(e, mce_con::conb_moment_arm(gk, xv));
            }
            E[(slot * kConChunkRows + row) * T::kStride + k] = e;
            if constexpr (kBounds)
                if (pmom[slot]) E[T::kPlane + (slot * kConChunkRows + row) * T::kStride + k] = m;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < kConChunkRows / 4; ++ks) {
            const int row = 4 * ks + frow;
            const double A = E[row * T::kStride + 16 * bi + fcol];
            double A1 = 0.0;
            if constexpr (kBounds)
                if (pmom[0]) A1 = E[T::kPlane + row * T::kStride + 16 * bi + fcol];
#pragma unroll
            for (int q = 0; q < kJB; ++q) {
                if (q < grp.cnt) {                               // (wave-uniform)
                    const double* er = E + ((1 + q) * kConChunkRows + row) * T::kStride + fcol;
#pragma unroll
                    for (int b = 0; b < T::kNbj; ++b) acc[0][q][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, er[16 * (bj0 + b)], acc[0][q][b], 0, 0, 0);
                    if constexpr (kBounds) {
                        if (pmom[0]) {                           // (wave-uniform) R_x += A' B
#pragma unroll
                            for (int b = 0; b < T::kNbj; ++b) acc[1][q][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(A1, er[16 * (bj0 + b)], acc[1][q][b], 0, 0, 0);
                        }
                        if (pmom[1 + q]) {                       // (wave-uniform) R_y += A B'
#pragma unroll
                            for (int b = 0; b < T::kNbj; ++b)
                                acc[2][q][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, er[T::kPlane + 16 * (bj0 + b)], acc[2][q][b], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // C/D of the fp64 MFMA: lane l holds column l & 15 and the rows (l >> 4) + 4 r
    const int P = mce_con::con_npairs(nc);
#pragma unroll
    for (int q = 0; q < kJB; ++q) {
        if (q < grp.cnt) {
#pragma unroll
            for (int z = 0; z < kSums; ++z) {
                if constexpr (kBounds) {
                    if (z == 1 && !pmom[0]) continue;
                    if (z == 2 && !pmom[1 + q]) continue;
                }
                double* out = S + (((csegs[y].part0 + part) * P + grp.pair0 + q) * kSums + z) * (int64_t)(G * G);
#pragma unroll
                for (int b = 0; b < T::kNbj; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) out[(16 * bi + frow + 4 * r) * G + 16 * (bj0 + b) + fcol] = acc[z][q][b][r];
            }
        }
    }
}

// the columns (s, t) of pair p
__device__ __forceinline__ void con_pair_cols(int p, int nc, int* s, int* t)
{
    int a = 0;
    while (p >= nc - 1 - a) { p -= nc - 1 - a; ++a; }
    *s = a;
    *t = a + 1 + p;
}

// grid: x = system * P + pair, y = block of 256 cells.  The densities go to the system's result block.  <true>: the three sums in part
// order each, then step 6" on prep's table
template <bool kBounds>
__global__ __launch_bounds__(kConThreads) void con_fold_kernel(const SumSeg* __restrict__ segs, const ConSeg* __restrict__ csegs, int nc, int np, int G,
                                                              const double* __restrict__ prm, const double* __restrict__ sys, const double* __restrict__ S,
                                                              const double* __restrict__ tab, double* __restrict__ res)
{
    constexpr int kPrm = ConForm<kBounds>::kPrm, kSums = ConForm<kBounds>::kSums;
    const int P = mce_con::con_npairs(nc), N = G * G;
    const int y = blockIdx.x / P, p = blockIdx.x - y * P;
    const int k = blockIdx.y * kConThreads + threadIdx.x;
    if (k >= N) return;
    int s, t;
    con_pair_cols(p, nc, &s, &t);
    const double* ps = prm + ((int64_t)y * nc + s) * kPrm;
    const double* pt = prm + ((int64_t)y * nc + t) * kPrm;
    double rho = __builtin_nan("");
    if ((int)ps[5] == mce_con::kConOk && (int)pt[5] == mce_con::kConOk) {
        const int nparts = mce_con::con_nparts(segs[y].n);
        const double* src = S + ((csegs[y].part0 * P + p) * kSums) * (int64_t)N + k;
        const int64_t pstride = (int64_t)P * kSums * N;           // from a part to the next
        double acc = 0.0;
        for (int q = 0; q < nparts; ++q) acc += src[q * pstride];
        const double norm = mce_con::con_norm(sys[(int64_t)y * kSumSys + 0], ps[0], pt[0]);
        rho = acc / norm;
        if constexpr (kBounds) {
            double rx = 0.0, ry = 0.0;                           // (a column that is open on both sides: +0.0, and nothing was written)
            if (!mce_con::conb_open(ps[8], ps[9]))
                for (int q = 0; q < nparts; ++q) rx += src[q * pstride + N];
            if (!mce_con::conb_open(pt[8], pt[9]))
                for (int q = 0; q < nparts; ++q) ry += src[q * pstride + 2 * (int64_t)N];
            const double* u = tab + (((int64_t)y * nc + s) * G + k / G) * kConTab;
            const double* v = tab + (((int64_t)y * nc + t) * G + k % G) * kConTab;
            rho = mce_con::conb_density(rho, mce_con::conb_t1(rx, ps[0], norm), mce_con::conb_t1(ry, pt[0], norm), u, v);
        }
    }
    con_dens_rows<kBounds>(res + csegs[y].out_off, nc, np)[(int64_t)p * N + k] = rho;
}

constexpr size_t con_region_lds_bytes(int G) { return (size_t)G * G * (2 * sizeof(double) + sizeof(int)); }

// grid: system * P + pair, one workgroup each; dynamic LDS: con_region_lds_bytes(G).  <true>: the running sum of step 8"; a failing pair
// takes its column's status, the x axis' first
template <bool kBounds>
__global__ __launch_bounds__(kConThreads) void con_region_kernel(const ConSeg* __restrict__ csegs, int nc, int np, int G, const double* __restrict__ prm,
                                                                const double* __restrict__ probs, double* __restrict__ res)
{
    extern __shared__ double con_lds[];
    __shared__ double red[kRedWaves];
    const int P = mce_con::con_npairs(nc), N = G * G;
    double* s_rho = con_lds;                                    // [N]
    double* s_cum = s_rho + N;                                  // [N]
    int* s_k = reinterpret_cast<int*>(s_cum + N);               // [N]
    const int y = blockIdx.x / P, p = blockIdx.x - y * P;
    int s, t;
    con_pair_cols(p, nc, &s, &t);
    const double* ps = prm + ((int64_t)y * nc + s) * ConForm<kBounds>::kPrm;
    const double* pt = prm + ((int64_t)y * nc + t) * ConForm<kBounds>::kPrm;
    double* block = res + csegs[y].out_off;
    double* pairr = con_pair_rows<kBounds>(block, nc) + p;
    double* pr = con_p_rows<kBounds>(block, nc) + p;
    const int cs = (int)ps[5], ct = (int)pt[5];
    const double nan = __builtin_nan("");
    if (cs != mce_con::kConOk || ct != mce_con::kConOk) {
        if (threadIdx.x == 0) {
            const bool failed = cs == kConSysFailed;
            pairr[mce_con::kConModeX * P] = nan;
            pairr[mce_con::kConModeY * P] = nan;
            pairr[mce_con::kConModeDensity * P] = nan;
            pairr[mce_con::kConPairStatus * P] = failed ? nan : (double)mce_con::conb_pair_status(cs, ct);
            for (int q = 0; q < np; ++q)
                for (int z = 0; z < mce_con::kConPerP; ++z) pr[(int64_t)(q * mce_con::kConPerP + z) * P] = (z == mce_con::kConCells && !failed) ? -1.0 : nan;
        }
        return;
    }
    const double lox = ps[2], stepx = ps[3], loy = pt[2], stepy = pt[3];
    const double* rho = con_dens_rows<kBounds>(block, nc, np) + (int64_t)p * N;
    for (int k = threadIdx.x; k < N; k += kConThreads) { s_rho[k] = rho[k]; s_k[k] = k; }
    __syncthreads();
    order_sort(s_rho, s_k, N);                                   // (N is a power of two)
    if (threadIdx.x == 0) {
        if constexpr (kBounds) {
            const bool x_lo = ps[10] != 0.0, x_hi = ps[11] != 0.0, y_lo = pt[10] != 0.0, y_hi = pt[11] != 0.0;
            order_running_sum(s_rho, s_k, N, s_cum, [=](double v, int k) { return mce_con::conb_weighted(v, k, G, x_lo, x_hi, y_lo, y_hi); });
        } else {
            order_running_sum(s_rho, N, s_cum);
        }
        pairr[mce_con::kConModeX * P] = mce_mar::mar_grid_point(lox, stepx, s_k[0] / G);
        pairr[mce_con::kConModeY * P] = mce_mar::mar_grid_point(loy, stepy, s_k[0] % G);
        pairr[mce_con::kConModeDensity * P] = s_rho[0];
        pairr[mce_con::kConPairStatus * P] = (double)mce_con::kConOk;
    }
    __syncthreads();
    const double Z = s_cum[N - 1];
    for (int q = 0; q < np; ++q) {
        const int cut = order_cut(s_cum, N, probs[q] * Z, red);
        double x0 = (double)G, x1 = -1.0, y0 = (double)G, y1 = -1.0, edge = 0.0;
        for (int i = threadIdx.x; i <= cut; i += kConThreads) {
            const int kx = s_k[i] / G, ky = s_k[i] % G;
            x0 = (double)kx < x0 ? (double)kx : x0;
            x1 = (double)kx > x1 ? (double)kx : x1;
            y0 = (double)ky < y0 ? (double)ky : y0;
            y1 = (double)ky > y1 ? (double)ky : y1;
            if (kx == 0 || kx == G - 1 || ky == 0 || ky == G - 1) edge = 1.0;
        }
        x0 = block_min(x0, red);
        x1 = block_max(x1, red);
        y0 = block_min(y0, red);
        y1 = block_max(y1, red);
        edge = block_max(edge, red);
        if (threadIdx.x == 0) {
            double* o = pr + (int64_t)q * mce_con::kConPerP * P;
            o[mce_con::kConLevel * P] = s_rho[cut];
            o[mce_con::kConCells * P] = (double)(cut + 1);
            o[mce_con::kConLowerX * P] = mce_mar::mar_grid_point(lox, stepx, (int)x0);
            o[mce_con::kConUpperX * P] = mce_mar::mar_grid_point(lox, stepx, (int)x1);
            o[mce_con::kConLowerY * P] = mce_mar::mar_grid_point(loy, stepy, (int)y0);
            o[mce_con::kConUpperY * P] = mce_mar::mar_grid_point(loy, stepy, (int)y1);
            o[mce_con::kConEdge * P] = edge;
        }
        __syncthreads();
    }
}

// one workgroup per system: the head and the column rows (<true>: and the bounds' rows)
template <bool kBounds>
__global__ __launch_bounds__(kConThreads) void con_result_kernel(const SumSeg* __restrict__ segs, const ConSeg* __restrict__ csegs, const int32_t* __restrict__ cols,
                                                                int nc, const double* __restrict__ sys, const double* __restrict__ col,
                                                                const double* __restrict__ prm, int G, int np, double* __restrict__ res)
{
    const int y = blockIdx.x;
    const SumSeg g = segs[y];
    const double* s = sys + (int64_t)y * kSumSys;
    double* out = res + csegs[y].out_off;
    if (threadIdx.x == 0) {
        int column;
        const int status = mar_sys_status(g, s, col, &column);
        mce_con::con_pack_head(status, column, s[0], s[1], s[2], G, np, nc, out);
    }
    const double nan = __builtin_nan("");
    double* c = con_col_rows(out);
    for (int t = threadIdx.x; t < nc; t += kConThreads) {
        const double* in = col + (g.col0 + cols[t]) * kSumCol;
        const double* p = prm + ((int64_t)y * nc + t) * ConForm<kBounds>::kPrm;
        const int cs = (int)p[5];
        const bool ok = cs == mce_con::kConOk;
        c[mce_con::kConCol * nc + t] = (double)cols[t];
        c[mce_con::kConMean * nc + t] = ok ? in[0] : nan;
        c[mce_con::kConVar * nc + t] = ok ? in[1] : nan;
        c[mce_con::kConSd * nc + t] = ok ? p[4] : nan;
        c[mce_con::kConH * nc + t] = ok ? p[0] : nan;
        c[mce_con::kConC * nc + t] = ok ? p[1] : nan;
        c[mce_con::kConLo * nc + t] = ok ? p[2] : nan;
        c[mce_con::kConStep * nc + t] = ok ? p[3] : nan;
        c[mce_con::kConColStatus * nc + t] = cs == kConSysFailed ? nan : (double)cs;
        if constexpr (kBounds) {
            c[mce_con::kConbBoundLo * nc + t] = cs == kConSysFailed ? nan : p[8];
            c[mce_con::kConbBoundHi * nc + t] = cs == kConSysFailed ? nan : p[9];
            c[mce_con::kConbAtLo * nc + t] = ok ? p[10] : nan;
            c[mce_con::kConbAtHi * nc + t] = ok ? p[11] : nan;
        }
    }
}

}  // namespace mce
