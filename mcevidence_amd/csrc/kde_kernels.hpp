// kde_kernels.hpp -- the leave-one-out kernel density sums behind shift="kde" (mce_kde_shift_dev, capi_kde.hpp) for difference chains
// that are on the device.  The rule is kde_shift.hpp's; this file arranges it into launches that serve any number of systems (one system
// = one (x, ld, n, d, w, linv, mean, point, c) segment) by the segment-tile scheme of seg_tiles.hpp, which states the invariant these
// launches keep.  Plain C++ stores only, no atomics, 64-bit row indices.
//
//   kde_whiten_kernel     per tile: z = linv (x - mean) of its rows, packed with the column count padded to a multiple of 4, and |z|^2; a
//                         row that is not used is written as zeros and nothing of it is read.  Per tile: sum w, sum w^2, the used rows,
//                         the bad weights, the lowest column with a bad value, and the point's sums S_0, Q_0.  The system's first tile
//                         writes the point's row z_0.
//   kde_sys_kernel        one workgroup per system: its tiles in block_fold's order: W, A2, rows, refusals, S_0, Q_0
//   kde_sum_kernel        the hot path.  A workgroup owns 64 query rows of ONE system (a wave 16 of them) and one PART of the system's
//                         reference rows, which it sweeps in chunks of 64 staged in LDS.  q . z of 16 queries x 16 references is a
//                         chain of v_mfma_f64_16x16x4_f64 over the d / 4 k-steps; then |q|^2 + |z|^2 - 2 q . z, the clamp, exp, times
//                         w_j with j == i masked; each lane adds into its four running sums in chunk order; a fixed shuffle tree over
//                         the 16 columns ends the part.  A 16 x 16 tile whose arguments are all at or above kKdeUnderflow is skipped: by
//                         the rule each of its terms is +0.0.  The parts' boundaries depend on n alone (kde_part_chunk).
//   kde_mass_tile_kernel  per tile: S_i = the parts in part order, t_i = S_i / (W - w_i), the four selection sums, the densities
//   kde_result_kernel     one workgroup per system: the tiles' selection sums by block_fold, the status, the result block
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "kde_shift.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kKdeThreads = kRedThreads;
constexpr int kKdeWaves = kRedWaves;
constexpr int kKdeTileHead = 7;                                 // per tile: sum w, sum w^2, used, bad weights, S_0, Q_0, lowest bad column
constexpr int kKdeSys = 8;                                      // per system: W, A2, used, bad weights, S_0, Q_0, lowest bad column, -
constexpr int kKdeMass = 4;                                     // per tile: M(t0), M(t0 - s0), M(t0 + s0), M_eq
constexpr int kKdeKSteps = mce_kde::kKdeMaxDim / 4;             // 16 A operands per lane at most
constexpr int kKdeSubTiles = mce_seg::kSegTileRows / mce_kde::kKdeChunkRows;
// LDS row stride of a staged reference row, in doubles, = 2 mod 32: a B fragment read (lane l: row l % 16, column 4 k + l / 16) is
// served in two halves of 32 lanes, whose 32 doubles (16 rows x 2 columns) then fall on the 64 banks once each
constexpr int kKdeLdsStride = mce_kde::kKdeMaxDim + 2;
constexpr double kKdeNoColumn = 1e9;
static_assert(mce_seg::kSegTileRows == 2 * kKdeThreads, "a thread holds two rows of its tile");
static_assert(mce_kde::kKdeChunkRows == 16 * kKdeWaves, "a wave owns 16 query rows of its workgroup's 64");

typedef double kde_v4d __attribute__((ext_vector_type(4)));

struct KdeSeg {
    const double* x;
    const double* w;
    double* dens;                                               // null, or n + 1 doubles
    double* zout;                                               // null, or n * d doubles
    int64_t ld, n;
    int64_t row0;                                               // the system's first row among the rows of the call
    int64_t zoff;                                               // of its whitened rows, in doubles
    int64_t par0;                                               // of linv[d * d], mean[d], point[d] in the call's parameter block
    double c;
    int32_t d, dpad;
};

// grid: the tiles.  z[zoff + i * dpad + k], zn[row0 + i], zp[system][kKdeMaxDim], head[tile][kKdeTileHead]
__global__ __launch_bounds__(kKdeThreads) void kde_whiten_kernel(const KdeSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg,
                                                                const double* __restrict__ par, double* __restrict__ z, double* __restrict__ zn,
                                                                double* __restrict__ zp, double* __restrict__ head)
{
    __shared__ double red[kKdeWaves];
    __shared__ double ls[mce_kde::kKdeMaxDim * mce_kde::kKdeMaxDim];
    __shared__ double ms[mce_kde::kKdeMaxDim], z0[mce_kde::kKdeMaxDim];
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const KdeSeg g = segs[s];
    const int d = g.d, dpad = g.dpad;
    const double* __restrict__ p = par + g.par0;
    for (int k = threadIdx.x; k < d * d; k += kKdeThreads) ls[k] = p[k];
    for (int k = threadIdx.x; k < d; k += kKdeThreads) ms[k] = p[d * d + k];
    __syncthreads();
    for (int k = threadIdx.x; k < d; k += kKdeThreads) {
        const double v = mce_kde::kde_whiten_coord(ls + k * d, p + d * d + d, ms, k);
        z0[k] = v;
        if (tile == tile0[s]) zp[s * mce_kde::kKdeMaxDim + k] = v;
    }
    __syncthreads();
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double badcol = kKdeNoColumn;
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const int64_t r = r0 + threadIdx.x + h * kKdeThreads;
        if (r >= r1) continue;
        const double a = g.w[r];
        const bool used = mce_sum::sum_used(a);
        double* __restrict__ zr = z + g.zoff + r * dpad;
        double* __restrict__ zo = g.zout ? g.zout + r * d : nullptr;
        double nn = 0.0, d0 = 0.0;
        if (used) {
            const double* __restrict__ xr = g.x + r * g.ld;
            for (int j = d - 1; j >= 0; --j)
                if (mce_sum::sum_value_bad(xr[j]) && (double)j < badcol) badcol = (double)j;
            for (int k = 0; k < d; ++k) {
                const double v = mce_kde::kde_whiten_coord(ls + k * d, xr, ms, k);
                zr[k] = v;
                if (zo) zo[k] = v;
                nn += v * v;
                const double e = v - z0[k];
                d0 += e * e;
            }
            for (int k = d; k < dpad; ++k) zr[k] = 0.0;
            const double wk = a * mce_kde::kde_kernel_value(g.c, d0);
            t[0] += a;
            t[1] += a * a;
            t[2] += 1.0;
            t[3] += mce_sum::sum_weight_bad(a) ? 1.0 : 0.0;
            t[4] += wk;
            t[5] += wk * wk;
        } else {
            for (int k = 0; k < dpad; ++k) zr[k] = 0.0;
            if (zo) for (int k = 0; k < d; ++k) zo[k] = 0.0;
        }
        zn[g.row0 + r] = nn;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double v = block_sum(t[k], red);
        if (threadIdx.x == 0) head[tile * kKdeTileHead + k] = v;
    }
    badcol = block_min(badcol, red);
    if (threadIdx.x == 0) head[tile * kKdeTileHead + 6] = badcol;
}

// one workgroup per system.  sys[y][kKdeSys]
__global__ __launch_bounds__(kKdeThreads) void kde_sys_kernel(const KdeSeg* __restrict__ segs, const int64_t* __restrict__ tile0, const double* __restrict__ head,
                                                             double* __restrict__ sys)
{
    __shared__ double red[kKdeWaves];
    const int y = blockIdx.x;
    const int64_t t0 = tile0[y], nt = mce_seg::seg_ntiles(segs[y].n);
    double tot[6];
    block_fold<6>(head + t0 * kKdeTileHead, nt, kKdeTileHead, tot, red);
    double badcol = kKdeNoColumn;
    for (int64_t k = threadIdx.x; k < nt; k += kKdeThreads) {
        const double b = head[(t0 + k) * kKdeTileHead + 6];
        badcol = b < badcol ? b : badcol;
    }
    badcol = block_min(badcol, red);
    if (threadIdx.x == 0) {
        double* out = sys + (int64_t)y * kKdeSys;
#pragma unroll
        for (int j = 0; j < 6; ++j) out[j] = tot[j];
        out[6] = badcol;
        out[7] = 0.0;
    }
}

// grid: tiles * kKdeSubTiles * pmax, pmax >= the parts of every system of the call; the workgroup (tile, sub, part) ends at once where
// its system has no such query rows or no such part.  partial[(row0 + i) * kKdeMaxParts + part]
__global__ __launch_bounds__(kKdeThreads) void kde_sum_kernel(const KdeSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int pmax,
                                                             const double* __restrict__ z, const double* __restrict__ zn, double* __restrict__ partial)
{
    __shared__ double zs[mce_kde::kKdeChunkRows * kKdeLdsStride];
    __shared__ double ns[mce_kde::kKdeChunkRows], ws[mce_kde::kKdeChunkRows];
    const int64_t unit = blockIdx.x / pmax;
    const int part = (int)(blockIdx.x - unit * pmax);
    const int64_t tile = unit / kKdeSubTiles;
    const int sub = (int)(unit - tile * kKdeSubTiles);
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const KdeSeg g = segs[s];
    const int64_t n = g.n, q0 = r0 + (int64_t)sub * mce_kde::kKdeChunkRows;
    if (q0 >= r1 || part >= mce_kde::kde_nparts(n)) return;
    const int dpad = g.dpad, nk = dpad >> 2;
    const double c = g.c;
    const double* __restrict__ zg = z + g.zoff;
    const double* __restrict__ zng = zn + g.row0;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fk = lane >> 4, fj = lane & 15;
    // A: lane l holds q[row l % 16][column 4 k + l / 16] of k-step k
    const int64_t qa_row = q0 + 16 * wv + fj;
    double qa[kKdeKSteps];
#pragma unroll
    for (int k = 0; k < kKdeKSteps; ++k) qa[k] = (k < nk && qa_row < n) ? zg[qa_row * dpad + 4 * k + fk] : 0.0;
    // C/D: lane l holds column l % 16 and the rows l / 16 + 4 r
    int64_t qrow[4];
    double qn[4], sum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        qrow[r] = q0 + 16 * wv + fk + 4 * r;
        qn[r] = qrow[r] < n ? zng[qrow[r]] : 0.0;
        sum[r] = 0.0;
    }
    const int64_t ch0 = mce_kde::kde_part_chunk(n, part), ch1 = mce_kde::kde_part_chunk(n, part + 1);
    for (int64_t ch = ch0; ch < ch1; ++ch) {
        const int64_t c0 = ch * mce_kde::kKdeChunkRows;
        __syncthreads();                                        // (the last chunk is read)
        for (int e = threadIdx.x; e < mce_kde::kKdeChunkRows * dpad; e += kKdeThreads) {
            const int row = e / dpad, col = e - row * dpad;
            zs[row * kKdeLdsStride + col] = c0 + row < n ? zg[(c0 + row) * dpad + col] : 0.0;
        }
        if (threadIdx.x < mce_kde::kKdeChunkRows) {
            const int64_t r = c0 + threadIdx.x;
            const double a = r < n ? g.w[r] : 0.0;
            ws[threadIdx.x] = mce_sum::sum_used(a) ? a : 0.0;
            ns[threadIdx.x] = r < n ? zng[r] : 0.0;
        }
        __syncthreads();
#pragma unroll 1
        for (int b = 0; b < mce_kde::kKdeChunkRows / 16; ++b) {
            if (c0 + 16 * b >= n) break;                        // (wave-uniform)
            const double* zb = zs + (16 * b + fj) * kKdeLdsStride + fk;
            kde_v4d acc = kde_v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k = 0; k < kKdeKSteps; ++k)
                if (k < nk) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(qa[k], zb[4 * k], acc, 0, 0, 0);
            const double znj = ns[16 * b + fj], wj = ws[16 * b + fj];
            const int64_t j = c0 + 16 * b + fj;
            double arg[4];
            bool live = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                arg[r] = c * mce_kde::kde_dist2(qn[r], znj, acc[r]);
                live = live || !(arg[r] >= mce_kde::kKdeUnderflow);
            }
            if (__builtin_amdgcn_ballot_w64(live) == 0) continue;  // every term of the 16 x 16 tile is +0.0 by the rule
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double term = wj * mce_kde::kde_kernel_arg_value(arg[r]);
                sum[r] += (j != qrow[r] && wj != 0.0) ? term : 0.0;
            }
        }
    }
    // the 16 columns of a row: a fixed tree
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) sum[r] += __shfl_xor(sum[r], o, 64);
        if (fj == 0 && qrow[r] < n) partial[(g.row0 + qrow[r]) * mce_kde::kKdeMaxParts + part] = sum[r];
    }
}

// grid: the tiles.  mass[tile][kKdeMass]
__global__ __launch_bounds__(kKdeThreads) void kde_mass_tile_kernel(const KdeSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg,
                                                                   const double* __restrict__ sys, const double* __restrict__ partial, double* __restrict__ mass)
{
    __shared__ double red[kKdeWaves];
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const KdeSeg g = segs[s];
    const double* y = sys + s * kKdeSys;
    const double W = y[0], t0 = y[4] / W, s0 = sqrt(y[5]) / W;
    const int np = mce_kde::kde_nparts(g.n);
    const double nan = __builtin_nan("");
    double M[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const int64_t r = r0 + threadIdx.x + h * kKdeThreads;
        if (r >= r1) continue;
        const double a = g.w[r];
        const bool used = mce_sum::sum_used(a);
        double t = nan;
        if (used) {
            const double* __restrict__ pp = partial + (g.row0 + r) * mce_kde::kKdeMaxParts;
            double S = 0.0;
            for (int p = 0; p < np; ++p) S += pp[p];
            t = S / (W - a);
            mce_kde::kde_select(t, a, t0, s0, M);
        }
        if (g.dens) g.dens[r] = t;
    }
#pragma unroll
    for (int k = 0; k < kKdeMass; ++k) {
        const double v = block_sum(M[k], red);
        if (threadIdx.x == 0) mass[tile * kKdeMass + k] = v;
    }
}

// one workgroup per system: res[y][kKdeOut]; a refused system's densities are overwritten with NaN
__global__ __launch_bounds__(kKdeThreads) void kde_result_kernel(const KdeSeg* __restrict__ segs, const int64_t* __restrict__ tile0, const double* __restrict__ sys,
                                                                const double* __restrict__ mass, double* __restrict__ res)
{
    __shared__ double red[kKdeWaves];
    __shared__ int sh_status;
    const int y = blockIdx.x;
    const KdeSeg g = segs[y];
    const double* s = sys + (int64_t)y * kKdeSys;
    double M[kKdeMass];
    block_fold<kKdeMass>(mass + tile0[y] * kKdeMass, mce_seg::seg_ntiles(g.n), kKdeMass, M, red);
    if (threadIdx.x == 0) {
        int column;
        const int status = mce_kde::kde_status(s[3] > 0.0, s[6] < kKdeNoColumn ? (int)s[6] : -1, s[0], s[2], &column);
        mce_kde::kde_pack(status, column, s[0], s[1], s[2], g.c, s[4], s[5], M, res + (int64_t)y * mce_kde::kKdeOut);
        sh_status = status;
    }
    __syncthreads();
    if (!g.dens) return;
    const double nan = __builtin_nan("");
    if (sh_status != mce_kde::kKdeOk) {
        for (int64_t i = threadIdx.x; i <= g.n; i += kKdeThreads) g.dens[i] = nan;
    } else if (threadIdx.x == 0) {
        g.dens[g.n] = s[4] / s[0];
    }
}

}  // namespace mce
