// like_moments_kernels.hpp -- the weighted moments of the likelihood column behind information= (mce_like_moments_dev,
// capi_moments.hpp) for columns that are already on the device.  The rule is like_moments.hpp's; this file arranges it into four
// launches that serve any number of systems (one system = one (fs, w, n) segment: the s1 partition of one root) by the segment-tile
// scheme of seg_tiles.hpp, which states the invariant these launches keep.  Plain C++ stores only.
//
//   mom_sum_tile_kernel      step 1, per tile: sum a, sum a f, sum a^2, the used rows, the rows status 3 refuses -- five block_sums
//   mom_centre_kernel        one workgroup per system: its tiles, thread t taking t, t + 256, .., then block_sum: W, c = S / W, the status
//   mom_var_tile_kernel      step 2, per tile: sum a (f - c)^2 about the system's computed c
//   mom_result_kernel        one workgroup per system: its tiles in the same order, v = sum / W, and the result block
//                            {W, c, v, A2, rows used, status} (NaN values where the status is not 0): everything the host wants
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "like_moments.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kMomThreads = kRedThreads;
constexpr int kMomTileRows = mce_seg::kSegTileRows;
constexpr int kMomTileSums = 5;                                 // per tile: sum a, sum a f, sum a^2, used rows, refused rows
constexpr int kMomSys = 5;                                      // per system after step 1: W, c, A2, used rows, status

struct MomSeg {
    const double* fs;
    const double* w;
    int64_t n;
};

// grid: the tiles.  sums[tile][kMomTileSums]
__global__ __launch_bounds__(kMomThreads) void mom_sum_tile_kernel(const MomSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg,
                                                                   double* __restrict__ sums)
{
    __shared__ double red[kMomThreads / 64];
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const double* __restrict__ fs = segs[s].fs;
    const double* __restrict__ w = segs[s].w;
    double sa = 0.0, saf = 0.0, saa = 0.0, cnt = 0.0, bad = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kMomThreads) {
        const double a = w[r];
        if (!mce_mom::mom_used(a)) continue;
        const double f = fs[r];
        sa += a;
        saf += a * f;
        saa += a * a;
        cnt += 1.0;
        bad += mce_mom::mom_row_bad(a, f) ? 1.0 : 0.0;
    }
    const double t[kMomTileSums] = {sa, saf, saa, cnt, bad};
#pragma unroll
    for (int k = 0; k < kMomTileSums; ++k) {
        const double v = block_sum(t[k], red);
        if (threadIdx.x == 0) sums[tile * kMomTileSums + k] = v;
    }
}

// one workgroup per system.  sys[y][kMomSys]
__global__ __launch_bounds__(kMomThreads) void mom_centre_kernel(const MomSeg* __restrict__ segs, const int64_t* __restrict__ tile0,
                                                                 const double* __restrict__ sums, double* __restrict__ sys)
{
    __shared__ double red[kMomThreads / 64];
    const int y = blockIdx.x;
    double tot[kMomTileSums];
    block_fold<kMomTileSums>(sums + tile0[y] * kMomTileSums, mce_seg::seg_ntiles(segs[y].n), kMomTileSums, tot, red);
    if (threadIdx.x == 0) {
        const double W = tot[0];
        double* out = sys + (int64_t)y * kMomSys;
        out[0] = W;
        out[1] = tot[1] / W;
        out[2] = tot[2];
        out[3] = tot[3];
        out[4] = (double)mce_mom::mom_status(tot[4] > 0.0, W);
    }
}

// grid: the tiles.  part[tile]
__global__ __launch_bounds__(kMomThreads) void mom_var_tile_kernel(const MomSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg,
                                                                   const double* __restrict__ sys, double* __restrict__ part)
{
    __shared__ double red[kMomThreads / 64];
    const int64_t tile = blockIdx.x;
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const double* __restrict__ fs = segs[s].fs;
    const double* __restrict__ w = segs[s].w;
    const double c = sys[s * kMomSys + 1];
    double sum = 0.0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kMomThreads) {
        const double a = w[r];
        if (mce_mom::mom_used(a)) sum += mce_mom::mom_term(a, fs[r], c);
    }
    const double v = block_sum(sum, red);
    if (threadIdx.x == 0) part[tile] = v;
}

// one workgroup per system.  res[y][MCE_MOMENTS_OUT]
__global__ __launch_bounds__(kMomThreads) void mom_result_kernel(const MomSeg* __restrict__ segs, const int64_t* __restrict__ tile0,
                                                                 const double* __restrict__ sys, const double* __restrict__ part, double* __restrict__ res)
{
    __shared__ double red[kMomThreads / 64];
    const int y = blockIdx.x;
    double V;
    block_fold<1>(part + tile0[y], mce_seg::seg_ntiles(segs[y].n), 1, &V, red);
    if (threadIdx.x == 0) {
        const double* in = sys + (int64_t)y * kMomSys;
        mce_mom::mom_pack((int)in[4], in[0], in[1], V / in[0], in[2], in[3], res + (int64_t)y * mce_mom::kMomOut);
    }
}

}  // namespace mce
