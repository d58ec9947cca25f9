// seg_tiles.hpp -- the segment-tile scheme of the per-system statistics kernels (like_moments_kernels.hpp, jack_group_kernels.hpp,
// param_summary_kernels.hpp), shared by the host check (tests/native/seg_tiles_check.cpp, plain C++17 under g++), the host side of the
// library and the device kernels (__host__ __device__ under hipcc).  docs/design/seg_tiles.md has the whole of it.
//
// A call serves a TABLE of segments; one system is one segment of n rows.  A TILE is kSegTileRows = 512 rows of ONE segment, counted
// from the segment's first row; the segments' tiles are numbered through in table order, tile0[s] being the first tile of segment s.
// A segment without rows owns no tile and shares its tile0 with the next one, so "the last segment whose tile0 is at or below the
// tile" is the owner and never an empty segment.
//
// THE INVARIANT.  A tile never spans two systems, and every sum is formed in an order that the system's own row count fixes: the rows
// of a tile by a fixed tree over the workgroup, then the system's seg_ntiles(n) tile values by ONE workgroup, thread t taking the
// tiles t, t + 256, .. in turn, then the same fixed tree (block_reduce.hpp: block_fold).  What that promises: two runs give the same
// bits, and a system's bits do not depend on its neighbours in the table, its position, the number of systems or the call -- a system
// in a farm wave has the bits of its own resident run.  No floating-point atomics, fp64 throughout, 64-bit row indices.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef MCE_HD
#define MCE_HD __host__ __device__
#endif
#else
#ifndef MCE_HD
#define MCE_HD
#endif
#endif

#include <vector>

namespace mce_seg {

constexpr int kSegTileRows = 512;
constexpr int64_t kSegMaxTiles = 0x7fffffffLL;                  // a launch's grid counts the tiles in 31 bits

// the tiles of a segment of n rows
MCE_HD inline int64_t seg_ntiles(int64_t n) { return (n + kSegTileRows - 1) / kSegTileRows; }
// no table of nseg segments with nrows rows in all has more tiles than this (what a workspace is sized for)
MCE_HD inline int64_t seg_max_tiles(int64_t nrows, int64_t nseg) { return nrows / kSegTileRows + nseg; }

// the last i in [0, n) with key(i) <= x; key(0) <= x is the caller's promise, and key is non-decreasing.  Among equal keys the last
// entry wins, which is what skips the entries that own nothing.
template <class I, class Key> MCE_HD inline I last_at_or_below(I n, int64_t x, Key key)
{
    I lo = 0, hi = n - 1;
    while (lo < hi) {
        const I mid = lo + ((hi - lo + 1) >> 1);
        if (key(mid) <= x) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the segment of tile `tile` and its rows [r0, r1) in the segment.  Seg has a member n.
template <class Seg>
MCE_HD inline int64_t seg_tile_rows(const Seg* __restrict__ segs, const int64_t* __restrict__ tile0, int nseg, int64_t tile, int64_t& r0, int64_t& r1)
{
    const int64_t s = last_at_or_below((int64_t)nseg, tile, [tile0](int64_t i) { return tile0[i]; });
    const int64_t n = segs[s].n;
    r0 = (tile - tile0[s]) * kSegTileRows;
    r1 = r0 + kSegTileRows < n ? r0 + kSegTileRows : n;
    return s;
}

// the host's table: add() the segments' row counts in table order
struct SegTable {
    std::vector<int64_t> tile0;
    int64_t ntiles = 0, nrows = 0;
    void add(int64_t n)
    {
        tile0.push_back(ntiles);
        ntiles += seg_ntiles(n);
        nrows += n;
    }
    bool fits() const { return ntiles <= kSegMaxTiles; }           // otherwise the call is refused
};

}  // namespace mce_seg
