// jack_group_kernels.hpp -- the bookkeeping of the delete-a-group jackknife for chains that stay on the device (mce_jack_groups_dev,
// mce_jack_leave_out_dev: capi_jackres.hpp).  The rule is jack_groups.hpp's; this file arranges it into launches that serve any number
// of systems (one system = the s1 partition of one root) by the segment-tile scheme of seg_tiles.hpp, which states the invariant these
// launches keep; it holds per (system, slot).  Plain C++ stores only.
//
// A thread holds the two rows t and t + 256 of its tile in registers; the loop over the slots b = -1, 0 .. G - 1 is wave-uniform, as in
// jack_partial_kernel, and a row enters slot b's sums by compare-and-select (g != b): no indexed private array, no scratch.  Every
// leave-out sum is the sum of the deleted set's own terms -- block_sum per tile, then a fixed-order pass over the system's tiles --
// never total - group.
//
//   jg_groups_kernel        one lane per row: the group of the row (jg_group)
//   jg_sum_tile_kernel      step 1, per tile and slot: rows, sum a, sum a f, sum a^2, used rows, refused rows -- six block_sums.  A slot
//                           whose group has no row in the tile has the terms of slot -1 and takes its values (the same bits); a group
//                           id outside [0, G) raises the call's flag
//   jg_centre_kernel        one workgroup per (system, slot): its tiles, thread t taking t, t + 256, .., then block_sum: rows, W,
//                           c = S / W, A2, used rows, the status
//   jg_var_tile_kernel      step 2, per tile and slot: sum a (f - c_b)^2 about the slot's own computed c_b (systems with an fs column)
//   jg_result_kernel        one workgroup per (system, slot): the tiles in the same order, v = sum / W, and the slot's result block
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "jack_groups.hpp"
#include "like_moments.hpp"
#include "seg_tiles.hpp"

namespace mce {

constexpr int kJgThreads = kRedThreads;
constexpr int kJgTileRows = mce_seg::kSegTileRows;
constexpr int kJgTileSums = 6;                                  // per tile and slot: rows, sum a, sum a f, sum a^2, used rows, refused rows
constexpr int kJgSys = 6;                                       // per system and slot after step 1: rows, W, c, A2, used rows, status
static_assert(kJgTileRows == 2 * kJgThreads, "a thread holds two rows of its tile");

struct JgGroupSeg {
    const int64_t* rows;          // NULL: row i is sample row i
    const int64_t* src;           // NULL: nothing was thinned
    const int64_t* part_first;    // [nparts], on the device
    int64_t nparts, n, N;
    int32_t G, by;
    int32_t* out;                 // [n]
};

struct JgSeg {
    const double* w;
    const double* fs;             // NULL: no moments
    const int32_t* g;
    int64_t n;
    int32_t G;
    int32_t slot0;                // the system's first slot in the packed result: sum of (G + 1) over the systems before it
};

// grid: blocks of kJgThreads rows, counted from every segment's first row (blk0[s]: the segment's first block)
__global__ __launch_bounds__(kJgThreads) void jg_groups_kernel(const JgGroupSeg* __restrict__ segs, const int64_t* __restrict__ blk0, int nseg)
{
    const int64_t blk = blockIdx.x;
    const int64_t s = mce_farm::last_at_or_below(blk0, nseg, blk);
    const JgGroupSeg sg = segs[s];
    const int64_t i = (blk - blk0[s]) * kJgThreads + threadIdx.x;
    if (i < sg.n) sg.out[i] = mce_jg::jg_group(i, sg.rows, sg.src, sg.part_first, sg.nparts, sg.N, sg.G, sg.by);
}

// the two rows of this thread in tile `tile`: weights, fs, groups (a row beyond the segment: a = 0, g = -2, which no slot test meets
// and no sum takes).  Returns the segment.
struct JgRows {
    double a0, a1, f0, f1;
    int g0, g1;
    bool live0, live1;
};

__device__ __forceinline__ int64_t jg_load_rows(const JgSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int64_t tile, JgRows& r)
{
    int64_t r0, r1;
    const int64_t s = mce_seg::seg_tile_rows(segs, tile0, nseg, tile, r0, r1);
    const double* __restrict__ w = segs[s].w;
    const double* __restrict__ fs = segs[s].fs;
    const int32_t* __restrict__ g = segs[s].g;
    const int64_t i0 = r0 + threadIdx.x, i1 = i0 + kJgThreads;
    r.live0 = i0 < r1;
    r.live1 = i1 < r1;
    r.a0 = r.live0 ? w[i0] : 0.0;
    r.a1 = r.live1 ? w[i1] : 0.0;
    r.g0 = r.live0 ? (int)g[i0] : -2;
    r.g1 = r.live1 ? (int)g[i1] : -2;
    // a row with a == 0 is skipped entirely: its f is never read
    r.f0 = (fs && r.live0 && mce_mom::mom_used(r.a0)) ? fs[i0] : 0.0;
    r.f1 = (fs && r.live1 && mce_mom::mom_used(r.a1)) ? fs[i1] : 0.0;
    return s;
}

// grid: the tiles.  sums[tile][Gmax + 1][kJgTileSums]; *bad_ids = 1.0 where a group id lies outside [0, G)
__global__ __launch_bounds__(kJgThreads) void jg_sum_tile_kernel(const JgSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int nslots,
                                                                 double* __restrict__ sums, double* __restrict__ bad_ids)
{
    __shared__ double red[kJgThreads / 64];
    __shared__ unsigned long long red64[kJgThreads / 64];
    const int64_t tile = blockIdx.x;
    JgRows r;
    const int64_t s = jg_load_rows(segs, tile0, nseg, tile, r);
    const int G = segs[s].G;
    const bool has_f = segs[s].fs != nullptr;
    if ((r.live0 && (r.g0 < 0 || r.g0 >= G)) || (r.live1 && (r.g1 < 0 || r.g1 >= G))) *bad_ids = 1.0;
    // the groups that have a row in this tile (ids outside [0, 64) set no bit: the call fails on them anyway)
    unsigned long long mine = 0;
    if (r.live0 && r.g0 >= 0 && r.g0 < 64) mine |= 1ull << r.g0;
    if (r.live1 && r.g1 >= 0 && r.g1 < 64) mine |= 1ull << r.g1;
    const unsigned long long present = block_or(mine, red64);
    const bool u0 = r.live0 && mce_mom::mom_used(r.a0), u1 = r.live1 && mce_mom::mom_used(r.a1);
    const double bad0 = (u0 && has_f && mce_mom::mom_row_bad(r.a0, r.f0)) ? 1.0 : 0.0;
    const double bad1 = (u1 && has_f && mce_mom::mom_row_bad(r.a1, r.f1)) ? 1.0 : 0.0;
    double* const out = sums + tile * (int64_t)nslots * kJgTileSums;
    double full[kJgTileSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};           // thread 0: slot -1's values
    for (int b = -1; b < G; ++b) {                                       // wave-uniform
        double* const o = out + (int64_t)(b + 1) * kJgTileSums;
        if (b >= 0 && !((present >> b) & 1ull)) {                        // no row of b here: the terms of slot -1
            if (threadIdx.x == 0) {
#pragma unroll
                for (int k = 0; k < kJgTileSums; ++k) o[k] = full[k];
            }
            continue;
        }
        const bool in0 = r.live0 && mce_jg::jg_in_slot(r.g0, b), in1 = r.live1 && mce_jg::jg_in_slot(r.g1, b);
        const bool t0 = in0 && u0, t1 = in1 && u1;
        const double x0 = t0 ? r.a0 : 0.0, x1 = t1 ? r.a1 : 0.0;
        const double t[kJgTileSums] = {(in0 ? 1.0 : 0.0) + (in1 ? 1.0 : 0.0),
                                       x0 + x1,
                                       (t0 ? r.a0 * r.f0 : 0.0) + (t1 ? r.a1 * r.f1 : 0.0),
                                       x0 * x0 + x1 * x1,
                                       (t0 ? 1.0 : 0.0) + (t1 ? 1.0 : 0.0),
                                       (in0 ? bad0 : 0.0) + (in1 ? bad1 : 0.0)};
#pragma unroll
        for (int k = 0; k < kJgTileSums; ++k) {
            const double v = block_sum(t[k], red);
            if (threadIdx.x == 0) {
                o[k] = v;
                if (b < 0) full[k] = v;
            }
        }
    }
}

// grid: (systems, Gmax + 1).  sys[system][Gmax + 1][kJgSys]
__global__ __launch_bounds__(kJgThreads) void jg_centre_kernel(const JgSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nslots,
                                                               const double* __restrict__ sums, double* __restrict__ sys)
{
    __shared__ double red[kJgThreads / 64];
    const int y = blockIdx.x, slot = blockIdx.y;
    if (slot > segs[y].G) return;
    double tot[kJgTileSums];
    block_fold<kJgTileSums>(sums + (tile0[y] * nslots + slot) * kJgTileSums, mce_seg::seg_ntiles(segs[y].n), (int64_t)nslots * kJgTileSums, tot, red);
    if (threadIdx.x == 0) {
        const double W = tot[1];
        double* out = sys + ((int64_t)y * nslots + slot) * kJgSys;
        out[0] = tot[0];
        out[1] = W;
        out[2] = tot[2] / W;
        out[3] = tot[3];
        out[4] = tot[4];
        out[5] = (double)mce_mom::mom_status(tot[5] > 0.0, W);
    }
}

// grid: the tiles.  part[tile][Gmax + 1]
__global__ __launch_bounds__(kJgThreads) void jg_var_tile_kernel(const JgSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int nslots,
                                                                 const double* __restrict__ sys, double* __restrict__ part)
{
    __shared__ double red[kJgThreads / 64];
    const int64_t tile = blockIdx.x;
    JgRows r;
    const int64_t s = jg_load_rows(segs, tile0, nseg, tile, r);
    if (!segs[s].fs) return;                                             // (uniform: no moments for this system)
    const int G = segs[s].G;
    const bool u0 = r.live0 && mce_mom::mom_used(r.a0), u1 = r.live1 && mce_mom::mom_used(r.a1);
    for (int b = -1; b < G; ++b) {                                       // wave-uniform
        const double c = sys[(s * nslots + (b + 1)) * kJgSys + 2];
        const bool t0 = u0 && mce_jg::jg_in_slot(r.g0, b), t1 = u1 && mce_jg::jg_in_slot(r.g1, b);
        const double x = (t0 ? mce_mom::mom_term(r.a0, r.f0, c) : 0.0) + (t1 ? mce_mom::mom_term(r.a1, r.f1, c) : 0.0);
        const double v = block_sum(x, red);
        if (threadIdx.x == 0) part[tile * (int64_t)nslots + (b + 1)] = v;
    }
}

// grid: (systems, Gmax + 1).  res[segs[y].slot0 + slot][MCE_JACK_LEAVE_OUT]
__global__ __launch_bounds__(kJgThreads) void jg_result_kernel(const JgSeg* __restrict__ segs, const int64_t* __restrict__ tile0, int nslots,
                                                               const double* __restrict__ sys, const double* __restrict__ part, double* __restrict__ res)
{
    __shared__ double red[kJgThreads / 64];
    const int y = blockIdx.x, slot = blockIdx.y;
    if (slot > segs[y].G) return;
    const bool moments = segs[y].fs != nullptr;
    double V;                                                            // (no moments: no tile is read)
    block_fold<1>(part + tile0[y] * nslots + slot, moments ? mce_seg::seg_ntiles(segs[y].n) : 0, nslots, &V, red);
    if (threadIdx.x == 0) {
        const double* in = sys + ((int64_t)y * nslots + slot) * kJgSys;
        mce_jg::jg_pack(moments, in[0], in[1], (int)in[5], in[1], in[2], V / in[1], in[3], in[4], res + ((int64_t)segs[y].slot0 + slot) * mce_jg::kJgOut);
    }
}

}  // namespace mce
