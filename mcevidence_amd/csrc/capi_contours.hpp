// capi_contours.hpp -- part of capi.hip (one translation unit): mce_param_contours_out_doubles / mce_param_contours_workspace_bytes /
// mce_param_contours_dev / mce_param_contours_f64: the 2-D joint densities, modes and credible regions of every pair of chosen
// parameter columns of MANY systems (the ready roots of a farm wave) that are on the device, in one call (param_contours_kernels.hpp has
// the launches, param_contours.hpp the rule).  Everything is enqueued on the caller's stream; the host waits once, for one block of
// results.  Argument checks come before any device call.  Ten launches, whatever the number of systems.
#pragma once

#include "capi_seg.hpp"
#include "param_contours.hpp"
#include "param_contours_kernels.hpp"

namespace {

constexpr int32_t kConMaxSegs = 1 << 16;
constexpr int64_t kConMaxRows = 0x7fffffffLL;

// no table of nseg segments with nrows rows has more (system, part) pairs than this
size_t con_max_parts(int64_t nrows_total, int32_t nseg)
{
    return (size_t)std::min<int64_t>((int64_t)mce_con::kConMaxParts * nseg, mce_seg::seg_max_tiles(nrows_total, nseg));
}

// the workspace of a call: nrows_total rows in nseg segments, at most dmax columns, nc chosen columns, np probabilities, G x G cells
struct ConWs {
    mce::SumSeg* segs;
    int64_t* tile0;
    double *head, *cols, *part, *sys, *col, *prm, *probs, *S, *res;
    mce::SumRun* runs;
    mce::ConSeg* csegs;
    mce::ConGroup* groups;
    int32_t* chosen;
    size_t total;
    ConWs(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t G, void* ws = nullptr)
    {
        const size_t Sg = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows_total, nseg), R = Sg * (size_t)dmax, D = (size_t)dmax;
        const size_t P = (size_t)mce_con::con_npairs(nc), N = (size_t)G * (size_t)G;
        WsPlan Pl(ws);
        segs = Pl.take<mce::SumSeg>(Sg);
        tile0 = Pl.take<int64_t>(Sg);
        head = Pl.take<double>(T * mce::kSumTileHead);
        cols = Pl.take<double>(T * mce::kSumTileCol * D);
        part = Pl.take<double>(T * D);
        sys = Pl.take<double>(Sg * mce::kSumSys);
        col = Pl.take<double>(R * mce::kSumCol);
        runs = Pl.take<mce::SumRun>(R);
        csegs = Pl.take<mce::ConSeg>(Sg);
        groups = Pl.take<mce::ConGroup>((size_t)mce_con::kConMaxPairs);
        chosen = Pl.take<int32_t>((size_t)mce_con::kConMaxCols);
        prm = Pl.take<double>(Sg * (size_t)nc * mce::kConPrm);
        probs = Pl.take<double>((size_t)mce_con::kConMaxP + 1);
        S = Pl.take<double>(con_max_parts(nrows_total, nseg) * P * N);
        res = Pl.take<double>(Sg * (size_t)mce_con::con_out_doubles(nc, np, G));
        total = Pl.total;
    }
};

struct ConTables {
    std::vector<mce::SumSeg> segs;
    std::vector<mce::ConSeg> csegs;
    std::vector<mce::ConGroup> groups;
    mce_seg::SegTable tiles;
    std::vector<mce::SumRun> runs;
    int64_t out_doubles = 0, parts = 0;
    int32_t dmax = 1, max_parts = 0;
};

bool con_shape_ok(int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t G)
{
    return nseg >= 1 && nseg <= kConMaxSegs && dmax >= 1 && dmax <= mce_mar::kMarMaxDim && mce_con::con_nc_ok(nc) && np >= 1 && np <= mce_con::kConMaxP &&
           mce_con::con_grid_ok(G);
}

// the argument checks of both forms, and the tables
int con_tables(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t G, double scale, ConTables& T)
{
    if (!segs || !probs || !cols) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kConMaxSegs) return fail(MCE_ERR_INVALID, "param contours: %d segments (1 .. %d expected)", nseg, kConMaxSegs);
    if (!mce_con::con_nc_ok(nc)) return fail(MCE_ERR_INVALID, "param contours: %d columns (2 .. %d expected)", nc, mce_con::kConMaxCols);
    for (int32_t t = 0; t < nc; ++t)
        if (cols[t] < 0 || (t > 0 && cols[t] <= cols[t - 1])) return fail(MCE_ERR_INVALID, "param contours: cols[%d] = %d (a strictly increasing list of columns >= 0 expected)", t, cols[t]);
    if (np < 1 || np > mce_con::kConMaxP) return fail(MCE_ERR_INVALID, "param contours: %d probabilities (1 .. %d expected)", np, mce_con::kConMaxP);
    for (int32_t t = 0; t < np; ++t)
        if (!(probs[t] > 0.0 && probs[t] < 1.0)) return fail(MCE_ERR_INVALID, "param contours: probability %d is %g (0 < p < 1 expected)", t, probs[t]);
    if (!mce_con::con_grid_ok(G)) return fail(MCE_ERR_INVALID, "param contours: grid=%d (32 or 64 expected)", G);
    if (!mce_mar::mar_pos_finite(scale)) return fail(MCE_ERR_INVALID, "param contours: scale=%g (finite and > 0 expected)", scale);
    T.segs.assign((size_t)nseg, mce::SumSeg{});
    T.csegs.assign((size_t)nseg, mce::ConSeg{});
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_summary_seg& g = segs[s];
        if (g.d < 1 || g.d > mce_mar::kMarMaxDim) return fail(MCE_ERR_INVALID, "param contours: segment %d has d=%d (1 .. %d expected)", s, g.d, mce_mar::kMarMaxDim);
        if (cols[nc - 1] >= g.d) return fail(MCE_ERR_INVALID, "param contours: column %d asked of segment %d with d=%d", cols[nc - 1], s, g.d);
        if (g.n < 0 || g.n > kConMaxRows || g.ld < g.d || (g.n > 0 && (!g.x || !g.w)))
            return fail(MCE_ERR_INVALID, "param contours: segment %d has %lld rows, ld=%lld, d=%d at x %s, w %s", s, (long long)g.n, (long long)g.ld, g.d,
                        g.x ? "valid" : "null", g.w ? "valid" : "null");
        mce::SumSeg& o = T.segs[(size_t)s];
        o.x = g.x; o.w = g.w; o.fs = nullptr; o.ld = g.ld; o.n = g.n; o.d = g.d; o.pad = 0;
        o.out_off = T.out_doubles;
        o.col0 = (int64_t)T.runs.size();
        T.csegs[(size_t)s] = mce::ConSeg{T.parts, T.out_doubles};
        const int nparts = mce_con::con_nparts(g.n);
        T.parts += nparts;
        T.max_parts = std::max(T.max_parts, (int32_t)nparts);
        T.out_doubles += mce_con::con_out_doubles(nc, np, G);
        T.tiles.add(g.n);
        T.dmax = std::max(T.dmax, g.d);
        for (int32_t j = 0; j < g.d; ++j) T.runs.push_back(mce::SumRun{0, 0, s, j});
    }
    if (!T.tiles.fits()) return fail(MCE_ERR_INVALID, "param contours: %lld rows in one call", (long long)T.tiles.nrows);
    // the groups: every x column with its partners, kConJB at a time
    for (int32_t s = 0; s + 1 < nc; ++s)
        for (int32_t t0 = s + 1; t0 < nc; t0 += mce::kConJB)
            T.groups.push_back(mce::ConGroup{s, t0, std::min<int32_t>(mce::kConJB, nc - t0), mce_con::con_pair_index(s, t0, nc)});
    return MCE_OK;
}

// the region kernel sorts in more LDS than the default limit, and so may the density kernel's staging: raise it once per device (a
// failure is not remembered)
int con_attr_once()
{
    static std::atomic<bool> attr_set[kMaxDevices];
    int dev = 0;
    MCE_HIP(hipGetDevice(&dev));
    if (dev >= kMaxDevices || !attr_set[dev].load()) {
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::con_region_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mce::con_region_lds_bytes(mce_con::kConMaxGrid)));
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::con_density_kernel<64>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mce::ConTile<64>::kLdsBytes));
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::con_density_kernel<32>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mce::ConTile<32>::kLdsBytes));
        if (dev < kMaxDevices) attr_set[dev].store(true);
    }
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_param_contours_out_doubles(int32_t nc, int32_t np, int32_t grid)
{
    if (!con_shape_ok(1, 1, nc, np, grid)) return 0;
    return (size_t)mce_con::con_out_doubles(nc, np, grid);
}

size_t mce_param_contours_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t grid)
{
    if (nrows_total < 0 || !con_shape_ok(nseg, dmax, nc, np, grid)) return 0;
    return ConWs(nrows_total, nseg, dmax, nc, np, grid).total;
}

int mce_param_contours_dev(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t grid, double scale,
                           double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    ConTables T;
    int rc = con_tables(segs, nseg, cols, nc, probs, np, grid, scale, T);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const ConWs W(T.tiles.nrows, nseg, T.dmax, nc, np, grid, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param contours", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    if ((size_t)T.parts > con_max_parts(T.tiles.nrows, nseg)) return fail(MCE_ERR_WORKSPACE, "param contours: %lld parts, fewer planned", (long long)T.parts);
    if ((rc = con_attr_once()) != MCE_OK) return rc;
    const int dmax = T.dmax, G = grid, P = mce_con::con_npairs(nc), ngroups = (int)T.groups.size();
    const int64_t R = (int64_t)T.runs.size();
    if (R > mce_seg::kSegMaxTiles || (int64_t)nseg * P > mce_seg::kSegMaxTiles) return fail(MCE_ERR_INVALID, "param contours: %lld columns in one call", (long long)R);
    MCE_HIP(hipMemcpyAsync(W.runs, T.runs.data(), T.runs.size() * sizeof(SumRun), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.csegs, T.csegs.data(), T.csegs.size() * sizeof(ConSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.groups, T.groups.data(), T.groups.size() * sizeof(ConGroup), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.chosen, cols, (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.probs, probs, (size_t)np * 8, hipMemcpyHostToDevice, st));
    const dim3 tb(kPsumThreads);
    const unsigned ntiles = (unsigned)T.tiles.ntiles;
    // the moments, by summary's kernels as they stand
    if (ntiles > 0) hipLaunchKernelGGL(sum_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.head, W.cols);
    hipLaunchKernelGGL(sum_sys_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.head, W.sys);
    hipLaunchKernelGGL(sum_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.cols, W.sys, W.col);
    if (ntiles > 0) hipLaunchKernelGGL(sum_var_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.col, W.part);
    hipLaunchKernelGGL(sum_var_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.part, W.sys, W.col);
    // the bandwidths and grids; the kernel products per part; the fold; the decisions; the blocks
    const dim3 ct(kConThreads);
    const int64_t ncols = (int64_t)nseg * nc;
    hipLaunchKernelGGL(con_prep_kernel, dim3((unsigned)((ncols + kConThreads - 1) / kConThreads)), ct, 0, st, W.segs, (int)nseg, W.chosen, (int)nc, W.sys, W.col, G, scale,
                       W.prm);
    if (T.max_parts > 0) {
        const dim3 dg((unsigned)((int64_t)nseg * ngroups), (unsigned)T.max_parts);
        if (G == 64) hipLaunchKernelGGL(con_density_kernel<64>, dg, ct, ConTile<64>::kLdsBytes, st, W.segs, W.csegs, W.groups, ngroups, W.chosen, (int)nc, W.prm, W.S);
        else hipLaunchKernelGGL(con_density_kernel<32>, dg, ct, ConTile<32>::kLdsBytes, st, W.segs, W.csegs, W.groups, ngroups, W.chosen, (int)nc, W.prm, W.S);
    }
    hipLaunchKernelGGL(con_fold_kernel, dim3((unsigned)(nseg * P), (unsigned)(G * G / kConThreads)), ct, 0, st, W.segs, W.csegs, (int)nc, (int)np, G, W.prm, W.sys, W.S,
                       W.res);
    hipLaunchKernelGGL(con_region_kernel, dim3((unsigned)(nseg * P)), ct, con_region_lds_bytes(G), st, W.csegs, (int)nc, (int)np, G, W.prm, W.probs, W.res);
    hipLaunchKernelGGL(con_result_kernel, dim3((unsigned)nseg), ct, 0, st, W.segs, W.csegs, W.chosen, (int)nc, W.sys, W.col, W.prm, G, (int)np, W.res);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, W.res, (size_t)T.out_doubles * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    return MCE_OK;
}

int mce_param_contours_f64(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t grid, double scale,
                           double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    ConTables T;
    int rc = con_tables(segs, nseg, cols, nc, probs, np, grid, scale, T);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    SegStage data;
    DevBuf ws;
    std::vector<mce_summary_seg> dsegs;
    if ((rc = seg_stage_xw(segs, nseg, data, dsegs)) != MCE_OK) return rc;
    for (mce_summary_seg& g : dsegs) g.fs = nullptr;             // (the likelihood column is not an input)
    const size_t wsb = mce_param_contours_workspace_bytes(T.tiles.nrows, nseg, T.dmax, nc, np, grid);
    MCE_HIP(ws.alloc(wsb));
    return mce_param_contours_dev(dsegs.data(), nseg, cols, nc, probs, np, grid, scale, out, ws.p, wsb, nullptr);
}

}  // extern "C"
