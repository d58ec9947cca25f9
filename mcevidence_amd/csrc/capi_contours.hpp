// capi_contours.hpp -- part of capi.hip (one translation unit): mce_param_contours_out_doubles / mce_param_contours_workspace_bytes /
// mce_param_contours_dev / mce_param_contours_f64: the 2-D joint densities, modes and credible regions of every pair of chosen
// parameter columns of MANY systems (the ready roots of a farm wave) that are on the device, in one call (param_contours_kernels.hpp has
// the launches, param_contours.hpp the rule).  Everything is enqueued on the caller's stream; the host waits once, for one block of
// results.  Argument checks come before any device call.  Ten launches, whatever the number of systems: the five of summary's moments
// (capi_sum_front.hpp: the head of the workspace, the per-segment checks and tables and these launches), then con_prep / con_density /
// con_fold / con_region / con_result.
//
// mce_param_contours_bounded_out_doubles / .._workspace_bytes / .._dev / .._f64 are the same for chains with hard prior bounds: per
// segment a HOST array bounds = lo[nc], then hi[nc] of the chosen columns (-inf / +inf: that side is open), which travels with the
// segment table.  ONE driver serves both (con_drive<kBounds>): the same ten launches of the kernels' <true> instances, the per-part sums
// tripled, and prep's table of boundary constants in the workspace.
#pragma once

#include "capi_sum_front.hpp"
#include "param_contours.hpp"
#include "param_contours_kernels.hpp"

namespace {

// no table of nseg segments with nrows rows has more (system, part) pairs than this
size_t con_max_parts(int64_t nrows_total, int32_t nseg)
{
    return (size_t)std::min<int64_t>((int64_t)mce_con::kConMaxParts * nseg, mce_seg::seg_max_tiles(nrows_total, nseg));
}

// the workspace of a call: nrows_total rows in nseg segments, at most dmax columns, nc chosen columns, np probabilities, G x G cells
struct ConWs : SumFrontWs {
    double *prm, *probs, *S, *res, *bnd = nullptr, *tab = nullptr;
    mce::ConSeg* csegs;
    mce::ConGroup* groups;
    int32_t* chosen;
    size_t total;
    ConWs(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t G, bool bounds, void* ws = nullptr)
    {
        const size_t prm_doubles = bounds ? mce::ConForm<true>::kPrm : mce::ConForm<false>::kPrm, sums = bounds ? mce::ConForm<true>::kSums : mce::ConForm<false>::kSums;
        const size_t Sg = (size_t)nseg, P = (size_t)mce_con::con_npairs(nc), N = (size_t)G * (size_t)G;
        WsPlan Pl(ws);
        take(Pl, nrows_total, nseg, dmax, true);
        csegs = Pl.take<mce::ConSeg>(Sg);
        groups = Pl.take<mce::ConGroup>((size_t)mce_con::kConMaxPairs);
        chosen = Pl.take<int32_t>((size_t)mce_con::kConMaxCols);
        prm = Pl.take<double>(Sg * (size_t)nc * prm_doubles);
        probs = Pl.take<double>((size_t)mce_con::kConMaxP + 1);
        S = Pl.take<double>(con_max_parts(nrows_total, nseg) * P * N * sums);
        res = Pl.take<double>(Sg * (size_t)(bounds ? mce_con::conb_out_doubles(nc, np, G) : mce_con::con_out_doubles(nc, np, G)));
        if (bounds) {
            bnd = Pl.take<double>(Sg * 2 * (size_t)nc);
            tab = Pl.take<double>(Sg * (size_t)nc * (size_t)G * mce::kConTab);
        }
        total = Pl.total;
    }
};

struct ConTables : SumFrontTables {
    std::vector<mce::ConSeg> csegs;
    std::vector<mce::ConGroup> groups;
    int64_t parts = 0;
    int32_t max_parts = 0;
};

bool con_shape_ok(int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t G)
{
    return nseg >= 1 && nseg <= kSumMaxSegs && dmax >= 1 && dmax <= mce_mar::kMarMaxDim && mce_con::con_nc_ok(nc) && np >= 1 && np <= mce_con::kConMaxP &&
           mce_con::con_grid_ok(G);
}

// the argument checks of both forms, and the tables
int con_tables(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t G, double scale, bool bounds,
               ConTables& T)
{
    const int32_t jb = bounds ? mce::ConForm<true>::kJB : mce::ConForm<false>::kJB;
    int rc = sum_front_args("param contours", segs && probs && cols, nseg);
    if (rc != MCE_OK) return rc;
    if (!mce_con::con_nc_ok(nc)) return fail(MCE_ERR_INVALID, "param contours: %d columns (2 .. %d expected)", nc, mce_con::kConMaxCols);
    for (int32_t t = 0; t < nc; ++t)
        if (cols[t] < 0 || (t > 0 && cols[t] <= cols[t - 1])) return fail(MCE_ERR_INVALID, "param contours: cols[%d] = %d (a strictly increasing list of columns >= 0 expected)", t, cols[t]);
    if (np < 1 || np > mce_con::kConMaxP) return fail(MCE_ERR_INVALID, "param contours: %d probabilities (1 .. %d expected)", np, mce_con::kConMaxP);
    for (int32_t t = 0; t < np; ++t)
        if (!(probs[t] > 0.0 && probs[t] < 1.0)) return fail(MCE_ERR_INVALID, "param contours: probability %d is %g (0 < p < 1 expected)", t, probs[t]);
    if (!mce_con::con_grid_ok(G)) return fail(MCE_ERR_INVALID, "param contours: grid=%d (32 or 64 expected)", G);
    if (!mce_mar::mar_pos_finite(scale)) return fail(MCE_ERR_INVALID, "param contours: scale=%g (finite and > 0 expected)", scale);
    rc = sum_front_tables(
        "param contours", segs, nseg, T,
        [&](int32_t s, const mce_summary_seg& g) {
            return cols[nc - 1] >= g.d ? fail(MCE_ERR_INVALID, "param contours: column %d asked of segment %d with d=%d", cols[nc - 1], s, g.d) : MCE_OK;
        },
        [&](int32_t, const mce_summary_seg& g) {
            T.csegs.push_back(mce::ConSeg{T.parts, T.out_doubles});
            const int nparts = mce_con::con_nparts(g.n);
            T.parts += nparts;
            T.max_parts = std::max(T.max_parts, (int32_t)nparts);
            return bounds ? mce_con::conb_out_doubles(nc, np, G) : mce_con::con_out_doubles(nc, np, G);
        });
    if (rc != MCE_OK) return rc;
    // the groups: every x column with its partners, kJB at a time
    for (int32_t s = 0; s + 1 < nc; ++s)
        for (int32_t t0 = s + 1; t0 < nc; t0 += jb)
            T.groups.push_back(mce::ConGroup{s, t0, std::min<int32_t>(jb, nc - t0), mce_con::con_pair_index(s, t0, nc)});
    return MCE_OK;
}

// the bounds of a call: nseg * 2 * nc doubles, every pair lo < hi (neither is NaN)
int con_bounds_ok(const double* bounds, int32_t nseg, int32_t nc)
{
    if (!bounds) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || !mce_con::con_nc_ok(nc)) return MCE_OK;      // (con_tables reports these)
    for (int32_t y = 0; y < nseg; ++y)
        for (int32_t t = 0; t < nc; ++t) {
            const double L = bounds[(size_t)y * 2 * nc + t], U = bounds[(size_t)y * 2 * nc + nc + t];
            if (!mce_marb::marb_bounds_ok(L, U)) return fail(MCE_ERR_INVALID, "param contours: bounds (%g, %g) of column %d of segment %d (lo < hi expected)", L, U, t, y);
        }
    return MCE_OK;
}

// the launches of both forms, on segments that are on the device.  T: con_tables' of the same arguments
template <bool kBounds>
int con_drive(ConTables& T, int32_t nseg, const int32_t* cols, int32_t nc, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale, double* out,
              void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    int rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const ConWs W(T.tiles.nrows, nseg, T.dmax, nc, np, grid, kBounds, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param contours", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    if ((size_t)T.parts > con_max_parts(T.tiles.nrows, nseg)) return fail(MCE_ERR_WORKSPACE, "param contours: %lld parts, fewer planned", (long long)T.parts);
    // the region kernel sorts in more LDS than the default limit, and so may the density kernel's staging
    static std::atomic<bool> attr_set[kMaxDevices];
    if ((rc = seg_attr_once(attr_set, {{reinterpret_cast<const void*>(con_region_kernel<kBounds>), con_region_lds_bytes(mce_con::kConMaxGrid)},
                                       {reinterpret_cast<const void*>(con_density_kernel<64, kBounds>), ConTile<64, kBounds>::kLdsBytes},
                                       {reinterpret_cast<const void*>(con_density_kernel<32, kBounds>), ConTile<32, kBounds>::kLdsBytes}})) != MCE_OK)
        return rc;
    const int G = grid, P = mce_con::con_npairs(nc), ngroups = (int)T.groups.size();
    const int64_t R = (int64_t)T.runs.size();
    if (R > mce_seg::kSegMaxTiles || (int64_t)nseg * P > mce_seg::kSegMaxTiles) return fail(MCE_ERR_INVALID, "param contours: %lld columns in one call", (long long)R);
    MCE_HIP(hipMemcpyAsync(W.csegs, T.csegs.data(), T.csegs.size() * sizeof(ConSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.groups, T.groups.data(), T.groups.size() * sizeof(ConGroup), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.chosen, cols, (size_t)nc * sizeof(int32_t), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.probs, probs, (size_t)np * 8, hipMemcpyHostToDevice, st));
    if constexpr (kBounds) MCE_HIP(hipMemcpyAsync(W.bnd, bounds, (size_t)nseg * 2 * (size_t)nc * 8, hipMemcpyHostToDevice, st));
    // the moments, by summary's kernels as they stand
    if ((rc = sum_front_launch(W, T, nseg, true, st)) != MCE_OK) return rc;
    // the bandwidths and grids; the kernel products per part; the fold; the decisions; the blocks
    const dim3 ct(kConThreads);
    const int64_t ncols = (int64_t)nseg * nc;
    hipLaunchKernelGGL(con_prep_kernel<kBounds>, dim3((unsigned)((ncols + kConThreads - 1) / kConThreads)), ct, 0, st, W.segs, (int)nseg, W.chosen, (int)nc, W.sys, W.col,
                       W.bnd, G, scale, W.prm, W.tab);
    if (T.max_parts > 0) {
        const dim3 dg((unsigned)((int64_t)nseg * ngroups), (unsigned)T.max_parts);
        constexpr size_t lds64 = ConTile<64, kBounds>::kLdsBytes, lds32 = ConTile<32, kBounds>::kLdsBytes;
        if (G == 64) hipLaunchKernelGGL((con_density_kernel<64, kBounds>), dg, ct, lds64, st, W.segs, W.csegs, W.groups, ngroups, W.chosen, (int)nc, W.prm, W.S);
        else hipLaunchKernelGGL((con_density_kernel<32, kBounds>), dg, ct, lds32, st, W.segs, W.csegs, W.groups, ngroups, W.chosen, (int)nc, W.prm, W.S);
    }
    hipLaunchKernelGGL(con_fold_kernel<kBounds>, dim3((unsigned)(nseg * P), (unsigned)(G * G / kConThreads)), ct, 0, st, W.segs, W.csegs, (int)nc, (int)np, G, W.prm, W.sys,
                       W.S, W.tab, W.res);
    hipLaunchKernelGGL(con_region_kernel<kBounds>, dim3((unsigned)(nseg * P)), ct, con_region_lds_bytes(G), st, W.csegs, (int)nc, (int)np, G, W.prm, W.probs, W.res);
    hipLaunchKernelGGL(con_result_kernel<kBounds>, dim3((unsigned)nseg), ct, 0, st, W.segs, W.csegs, W.chosen, (int)nc, W.sys, W.col, W.prm, G, (int)np, W.res);
    return seg_dev_end(out, W.res, (size_t)T.out_doubles, st);
}

// the host form of both: the segments uploaded, then con_drive
template <bool kBounds>
int con_host(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
             double* out, int32_t device)
{
    ConTables T;
    int rc = con_tables(segs, nseg, cols, nc, probs, np, grid, scale, kBounds, T);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    SegStage data;
    DevBuf ws;
    std::vector<mce_summary_seg> dsegs;
    if ((rc = seg_stage_xw(segs, nseg, data, dsegs)) != MCE_OK) return rc;
    for (mce_summary_seg& g : dsegs) g.fs = nullptr;             // (the likelihood column is not an input)
    const size_t wsb = ConWs(T.tiles.nrows, nseg, T.dmax, nc, np, grid, kBounds).total;
    MCE_HIP(ws.alloc(wsb));
    ConTables D;
    if ((rc = con_tables(dsegs.data(), nseg, cols, nc, probs, np, grid, scale, kBounds, D)) != MCE_OK) return rc;
    return con_drive<kBounds>(D, nseg, cols, nc, bounds, probs, np, grid, scale, out, ws.p, wsb, nullptr);
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
    return ConWs(nrows_total, nseg, dmax, nc, np, grid, false).total;
}

int mce_param_contours_dev(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t grid, double scale,
                           double* out, void* ws, size_t ws_bytes, void* stream)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    ConTables T;
    const int rc = con_tables(segs, nseg, cols, nc, probs, np, grid, scale, false, T);
    if (rc != MCE_OK) return rc;
    return con_drive<false>(T, nseg, cols, nc, nullptr, probs, np, grid, scale, out, ws, ws_bytes, stream);
}

int mce_param_contours_f64(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* probs, int32_t np, int32_t grid, double scale,
                           double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    return con_host<false>(segs, nseg, cols, nc, nullptr, probs, np, grid, scale, out, device);
}

size_t mce_param_contours_bounded_out_doubles(int32_t nc, int32_t np, int32_t grid)
{
    if (!con_shape_ok(1, 1, nc, np, grid)) return 0;
    return (size_t)mce_con::conb_out_doubles(nc, np, grid);
}

size_t mce_param_contours_bounded_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t nc, int32_t np, int32_t grid)
{
    if (nrows_total < 0 || !con_shape_ok(nseg, dmax, nc, np, grid)) return 0;
    return ConWs(nrows_total, nseg, dmax, nc, np, grid, true).total;
}

int mce_param_contours_bounded_dev(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* bounds, const double* probs, int32_t np,
                                   int32_t grid, double scale, double* out, void* ws, size_t ws_bytes, void* stream)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    ConTables T;
    int rc = con_tables(segs, nseg, cols, nc, probs, np, grid, scale, true, T);
    if (rc != MCE_OK) return rc;
    if ((rc = con_bounds_ok(bounds, nseg, nc)) != MCE_OK) return rc;
    return con_drive<true>(T, nseg, cols, nc, bounds, probs, np, grid, scale, out, ws, ws_bytes, stream);
}

int mce_param_contours_bounded_f64(const mce_summary_seg* segs, int32_t nseg, const int32_t* cols, int32_t nc, const double* bounds, const double* probs, int32_t np,
                                   int32_t grid, double scale, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    ConTables T;
    int rc = con_tables(segs, nseg, cols, nc, probs, np, grid, scale, true, T);
    if (rc != MCE_OK) return rc;
    if ((rc = con_bounds_ok(bounds, nseg, nc)) != MCE_OK) return rc;
    return con_host<true>(segs, nseg, cols, nc, bounds, probs, np, grid, scale, out, device);
}

}  // extern "C"
