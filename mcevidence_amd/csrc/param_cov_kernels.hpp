// param_cov_kernels.hpp -- the weighted parameter covariance behind covariance= (mce_param_cov_dev, capi_cov.hpp) for chains that are
// already on the device.  The rule is param_cov.hpp's; this file arranges it into launches that serve any number of systems (one system
// = one (x, ld, n, d, w) segment: the s1 partition of one root) by the segment-tile scheme of seg_tiles.hpp, which states the invariant
// these launches keep.  Plain C++ stores only, no atomics.
//
//   (sum_tile_kernel, sum_sys_kernel, sum_col_kernel of param_summary_kernels.hpp, as they stand, with fs = NULL: W, A2, the used
//    rows, the refusals and the means m_j -- bit for bit what mce_param_summary_dev forms)
//   cov_gram_kernel      per tile: the centred Gram matrix sum a (x_i - m_i)(x_j - m_j) of the tile's rows, as the 16 x 16 blocks of its
//                        upper triangle, each a chain of v_mfma_f64_16x16x4_f64 over the rows in row order
//   cov_fold_kernel      one workgroup per (system, block): thread t adds entry t of the system's tiles in tile order, divides by W and
//                        writes the entries inside d into the packed upper triangle of the result block
//   cov_result_kernel    one workgroup per system: the status and its precedence, the head, the means, the NaN fill
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "param_cov.hpp"
#include "param_summary_kernels.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kPcovThreads = kRedThreads;
constexpr int kPcovWaves = kRedWaves;
constexpr int kPcovChunkRows = 64;                               // rows of a tile staged in LDS at a time: 16 k-steps of 4 rows
constexpr int kPcovColsPad = 128;                                // 8 column blocks of 16
// LDS row stride in doubles, = 16 mod 32: a fragment read (lane l: row k0 + l / 16, column 16 b + l % 16) is served in two halves of
// 32 lanes, rows k0, k0 + 1 and k0 + 2, k0 + 3; the two rows of a half lie 144 doubles = 16 doubles mod 32 apart, so the half's 32
// doubles fall on the 64 banks once each
constexpr int kPcovLdsStride = kPcovColsPad + 16;
constexpr int kPcovBlocksPerWave = (mce_cov::kCovMaxBlocks + kPcovWaves - 1) / kPcovWaves;           // 9: 72 accumulator VGPRs
constexpr int kPcovBlockDoubles = mce_cov::kCovBlock * mce_cov::kCovBlock;
static_assert(mce_seg::kSegTileRows % kPcovChunkRows == 0 && kPcovChunkRows % 4 == 0, "a tile is whole chunks, a chunk whole k-steps");
static_assert(kPcovBlockDoubles == kPcovThreads, "the fold's thread t owns entry t of a block");

typedef double cov_v4d __attribute__((ext_vector_type(4)));

constexpr size_t cov_gram_lds_bytes() { return ((size_t)kPcovChunkRows * kPcovLdsStride + kPcovChunkRows + kPcovColsPad) * sizeof(double); }

// grid: the tiles.  gram[tile][nblkmax][256]: block p of the tile's own system (param_cov.hpp: cov_block), entry (i, j) of the block at
// 16 i + j.  Output block p belongs to wave p % 4, which keeps it in registers over the whole tile.  A chunk of 64 rows is written to
// LDS centred, y = x - m; a padding column >= d, a row past the segment's end and a row with a == 0 are written as ZEROS (their values
// are never read), and so is their weight.  Then per k-step of four rows and per block: A = a_r y_ri, B = y_rj.
__global__ __launch_bounds__(kPcovThreads) void cov_gram_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int nblkmax,
                                                              const double* __restrict__ col, double* __restrict__ gram)
{
    extern __shared__ double cov_lds[];
    double* ys = cov_lds;                                       // [kPcovChunkRows][kPcovLdsStride]
    double* as = ys + kPcovChunkRows * kPcovLdsStride;            // [kPcovChunkRows]
    double* ms = as + kPcovChunkRows;                            // [kPcovColsPad]
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const SumSeg g = segs[s];
    const int d = g.d;
    const int nb = mce_cov::cov_nblk(d), nblk = mce_cov::cov_nblocks(d), dpad = nb * mce_cov::kCovBlock;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int j = threadIdx.x; j < dpad; j += kPcovThreads) ms[j] = j < d ? col[(g.col0 + j) * kSumCol + 0] : 0.0;
    int bi[kPcovBlocksPerWave], bj[kPcovBlocksPerWave];
    cov_v4d acc[kPcovBlocksPerWave];
#pragma unroll
    for (int q = 0; q < kPcovBlocksPerWave; ++q) {
        bi[q] = 0;
        bj[q] = 0;
        if (wv + kPcovWaves * q < nblk) mce_cov::cov_block(wv + kPcovWaves * q, nb, &bi[q], &bj[q]);
        acc[q] = cov_v4d{0.0, 0.0, 0.0, 0.0};
    }
    const int frow = lane >> 4, fcol = lane & 15;
    const int srow = threadIdx.x >> 4, scol = threadIdx.x & 15;  // the staging thread's first row and column
    for (int64_t c0 = r0; c0 < r1; c0 += kPcovChunkRows) {
        __syncthreads();                                        // (the means are written; the last chunk is read)
        // 16 lanes take 16 consecutive columns of a row, the 16 groups of lanes the rows srow, srow + 16, ..: a row's weight is loaded once
        // per group, its columns block after block
        for (int row = srow; row < kPcovChunkRows; row += kPcovThreads / mce_cov::kCovBlock) {
            const int64_t r = c0 + row;
            const double a = r < r1 ? g.w[r] : 0.0;
            const bool used = mce_sum::sum_used(a);
            const double* __restrict__ xr = g.x + r * g.ld;
            for (int c = scol; c < dpad; c += mce_cov::kCovBlock) ys[row * kPcovLdsStride + c] = (used && c < d) ? xr[c] - ms[c] : 0.0;
            if (scol == 0) as[row] = used ? a : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < kPcovChunkRows / 4; ++ks) {
            const int row = 4 * ks + frow;
            const double a = as[row];
            const double* yr = ys + row * kPcovLdsStride + fcol;
#pragma unroll
            for (int q = 0; q < kPcovBlocksPerWave; ++q) {
                if (wv + kPcovWaves * q < nblk) {                // (wave-uniform)
                    const double A = a * yr[mce_cov::kCovBlock * bi[q]];
                    const double B = yr[mce_cov::kCovBlock * bj[q]];
                    acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, acc[q], 0, 0, 0);
                }
            }
        }
    }
    // C/D of the fp64 MFMA: lane l holds column l & 15 and the rows (l >> 4) + 4 r
#pragma unroll
    for (int q = 0; q < kPcovBlocksPerWave; ++q) {
        const int p = wv + kPcovWaves * q;
        if (p < nblk) {
            double* out = gram + (tile * nblkmax + p) * kPcovBlockDoubles;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(frow + 4 * r) * mce_cov::kCovBlock + fcol] = acc[q][r];
        }
    }
}

// grid: nseg * nblkmax, one workgroup per (system, block); a block the system does not have ends at once.  Thread t adds entry t of the
// system's tiles in tile order: the order depends on the system's row count alone.
__global__ __launch_bounds__(kPcovThreads) void cov_fold_kernel(const SumSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nblkmax,
                                                              const double* __restrict__ gram, const double* __restrict__ sys, double* __restrict__ res)
{
    const int y = blockIdx.x / nblkmax, p = blockIdx.x - y * nblkmax;
    const SumSeg g = segs[y];
    const int d = g.d, nb = mce_cov::cov_nblk(d);
    if (p >= mce_cov::cov_nblocks(d)) return;
    const int64_t t0 = tile0[y], nt = mce_seg::seg_ntiles(g.n);
    const double* in = gram + (t0 * nblkmax + p) * kPcovBlockDoubles + threadIdx.x;
    double acc = 0.0;
    for (int64_t k = 0; k < nt; ++k) acc += in[k * nblkmax * kPcovBlockDoubles];
    int bi, bj;
    mce_cov::cov_block(p, nb, &bi, &bj);
    const int i = mce_cov::kCovBlock * bi + (threadIdx.x >> 4), j = mce_cov::kCovBlock * bj + (threadIdx.x & 15);
    if (i <= j && j < d) res[g.out_off + mce_cov::kCovHead + d + mce_cov::cov_tri(i, j, d)] = acc / sys[(int64_t)y * kSumSys + 0];
}

// one workgroup per system: the result block (the fold has written the covariance of every system; a refused system's is overwritten)
__global__ __launch_bounds__(kPcovThreads) void cov_result_kernel(const SumSeg* __restrict__ segs, const double* __restrict__ sys, const double* __restrict__ col,
                                                                double* __restrict__ res)
{
    __shared__ int sh_status;
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
        const int status = mce_sum::sum_status((flags & 1) != 0, false, badcol, s[0], &column);
        mce_cov::cov_pack_head(status, column, s[0], s[1], s[2], out);
        sh_status = status;
    }
    __syncthreads();
    const bool ok = sh_status == mce_sum::kSumOk;
    const double nan = __builtin_nan("");
    double* mean = out + mce_cov::kCovHead;
    for (int j = threadIdx.x; j < g.d; j += kPcovThreads) mean[j] = ok ? col[(g.col0 + j) * kSumCol + 0] : nan;
    if (!ok) {
        const int64_t nt = mce_cov::cov_tri_doubles(g.d);
        for (int64_t k = threadIdx.x; k < nt; k += kPcovThreads) mean[g.d + k] = nan;
    }
}

}  // namespace mce
