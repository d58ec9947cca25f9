// capi_moments.hpp -- part of capi.hip (one translation unit): mce_like_moments_workspace_bytes / mce_like_moments_dev /
// mce_like_moments_f64: the weighted moments of the likelihood column of MANY systems (the ready roots of a farm wave) that are on the
// device, in one call (like_moments_kernels.hpp has the four launches, like_moments.hpp the rule).  Everything is enqueued on the
// caller's stream; the host waits once, for one block of results.  Argument checks come before any device call.
#pragma once

#include "capi_seg.hpp"
#include "like_moments.hpp"
#include "like_moments_kernels.hpp"

namespace {

// the workspace of a call of nseg segments with nrows rows in all
struct MomWs {
    mce::MomSeg* segs;
    int64_t* tile0;
    double *sums, *part, *sys, *res;
    size_t total;
    MomWs(int64_t nrows, int32_t nseg, void* ws = nullptr)
    {
        const size_t S = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows, nseg);
        WsPlan P(ws);
        segs = P.take<mce::MomSeg>(S);
        tile0 = P.take<int64_t>(S);
        sums = P.take<double>(T * mce::kMomTileSums);
        part = P.take<double>(T);
        sys = P.take<double>(S * mce::kMomSys);
        res = P.take<double>(S * mce_mom::kMomOut);
        total = P.total;
    }
};

constexpr int32_t kMomMaxSegs = 1 << 20;

// the argument checks of both forms, and the tables
int mom_tables(const mce_moments_seg* segs, int32_t nseg, std::vector<mce::MomSeg>& table, mce_seg::SegTable& tiles)
{
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kMomMaxSegs) return fail(MCE_ERR_INVALID, "like moments: %d segments (1 .. %d expected)", nseg, kMomMaxSegs);
    table.assign((size_t)nseg, mce::MomSeg{nullptr, nullptr, 0});
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_moments_seg& g = segs[s];
        if (g.n < 0 || g.n > (int64_t)1 << 40 || (g.n > 0 && (!g.fs || !g.w)))
            return fail(MCE_ERR_INVALID, "like moments: segment %d has %lld rows at fs %s, w %s", s, (long long)g.n, g.fs ? "valid" : "null", g.w ? "valid" : "null");
        table[(size_t)s] = mce::MomSeg{g.fs, g.w, g.n};
        tiles.add(g.n);
    }
    if (!tiles.fits()) return fail(MCE_ERR_INVALID, "like moments: %lld rows in one call", (long long)tiles.nrows);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_like_moments_workspace_bytes(int64_t nrows_total, int32_t nseg)
{
    if (nrows_total < 0 || nseg < 1 || nseg > kMomMaxSegs) return 0;
    return MomWs(nrows_total, nseg).total;
}

int mce_like_moments_dev(const mce_moments_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<MomSeg> table;
    mce_seg::SegTable tiles;
    int rc = mom_tables(segs, nseg, table, tiles);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    const MomWs W(tiles.nrows, nseg, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("like moments", ws_bytes, W.total, table, tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;

    const dim3 tb(kMomThreads), per_tile((unsigned)tiles.ntiles), per_sys((unsigned)nseg);
    if (tiles.ntiles > 0) hipLaunchKernelGGL(mom_sum_tile_kernel, per_tile, tb, 0, st, W.segs, W.tile0, (int)nseg, W.sums);
    hipLaunchKernelGGL(mom_centre_kernel, per_sys, tb, 0, st, W.segs, W.tile0, W.sums, W.sys);
    if (tiles.ntiles > 0) hipLaunchKernelGGL(mom_var_tile_kernel, per_tile, tb, 0, st, W.segs, W.tile0, (int)nseg, W.sys, W.part);
    hipLaunchKernelGGL(mom_result_kernel, per_sys, tb, 0, st, W.segs, W.tile0, W.sys, W.part, W.res);
    return seg_dev_end(out, W.res, (size_t)nseg * mce_mom::kMomOut, st);
}

int mce_like_moments_f64(const mce_moments_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<mce::MomSeg> table;
    mce_seg::SegTable tiles;
    int rc = mom_tables(segs, nseg, table, tiles);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    SegStage cols;
    DevBuf ws;
    if ((rc = cols.alloc((size_t)tiles.nrows * 2 * sizeof(double))) != MCE_OK) return rc;
    std::vector<mce_moments_seg> dsegs(segs, segs + nseg);
    for (mce_moments_seg& g : dsegs)
        if ((rc = cols.put(g.fs, (size_t)g.n, g.fs)) != MCE_OK || (rc = cols.put(g.w, (size_t)g.n, g.w)) != MCE_OK) return rc;
    const size_t wsb = mce_like_moments_workspace_bytes(tiles.nrows, nseg);
    MCE_HIP(ws.alloc(wsb));
    return mce_like_moments_dev(dsegs.data(), nseg, out, ws.p, wsb, nullptr);
}

}  // extern "C"
