// capi_marginals.hpp -- part of capi.hip (one translation unit): mce_param_marginals_out_doubles / mce_param_marginals_workspace_bytes /
// mce_param_marginals_dev / mce_param_marginals_f64 and their mce_param_marginals_bounded_.. forms: the 1-D marginal densities, modes
// and highest-density regions of the parameter columns of MANY systems (the ready roots of a farm wave) that are on the device, in one
// call, without and with hard prior bounds (param_marginals_kernels.hpp has the launches, param_marginals.hpp and
// param_marginals_bounds.hpp the rules).  The two families share every line here but their kernels' instance: kBounds.  The bounds are
// a HOST array that travels with the segment table.  Everything is enqueued on the caller's stream; the host waits once, for one block
// of results.  Argument checks come before any device call.  Ten launches, whatever the number of systems: the five of summary's
// moments (capi_sum_front.hpp: the head of the workspace, the per-segment checks and tables and these launches), then mar_prep /
// mar_density / mar_fold / mar_hpd / mar_result.
#pragma once

#include "capi_sum_front.hpp"
#include "param_marginals.hpp"
#include "param_marginals_bounds.hpp"
#include "param_marginals_kernels.hpp"

namespace {

// no table of nseg segments with nrows rows has more (system, part) pairs than this
size_t mar_max_parts(int64_t nrows_total, int32_t nseg)
{
    return (size_t)std::min<int64_t>((int64_t)mce_mar::kMarMaxParts * nseg, mce_seg::seg_max_tiles(nrows_total, nseg));
}

int64_t mar_block_doubles(bool bounded, int d, int np, int G) { return bounded ? mce_marb::marb_out_doubles(d, np, G) : mce_mar::mar_out_doubles(d, np, G); }

// the workspace of a call: nrows_total rows in nseg segments, at most dmax columns, np probabilities, G grid points.  bounded: the wider
// prm rows, the bounds, two sums per part and the wider blocks
struct MarWs : SumFrontWs {
    double *prm, *bnd, *probs, *S, *res;
    mce::MarSeg* msegs;
    size_t total;
    MarWs(bool bounded, int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t G, void* ws = nullptr)
    {
        const size_t Sg = (size_t)nseg, R = Sg * (size_t)dmax, D = (size_t)dmax;
        const size_t prm_w = bounded ? mce::MarForm<true>::kPrm : mce::MarForm<false>::kPrm;
        const size_t sums = bounded ? mce::MarForm<true>::kSums : mce::MarForm<false>::kSums;
        WsPlan P(ws);
        take(P, nrows_total, nseg, dmax, true);
        msegs = P.take<mce::MarSeg>(Sg);
        prm = P.take<double>(R * prm_w);
        bnd = P.take<double>(bounded ? R * 2 : 0);
        probs = P.take<double>((size_t)mce_mar::kMarMaxP + 1);
        S = P.take<double>(mar_max_parts(nrows_total, nseg) * D * sums * (size_t)G);
        res = P.take<double>(Sg * (size_t)mar_block_doubles(bounded, dmax, np, G));
        total = P.total;
    }
};

struct MarTables : SumFrontTables {
    std::vector<mce::MarSeg> msegs;
    std::vector<double> bnd;                                    // with bounds: per run L, U
    int64_t parts = 0;
    int32_t max_parts = 0;
};

bool mar_shape_ok(int32_t nseg, int32_t dmax, int32_t np, int32_t G)
{
    return nseg >= 1 && nseg <= kSumMaxSegs && dmax >= 1 && dmax <= mce_mar::kMarMaxDim && np >= 1 && np <= mce_mar::kMarMaxP && mce_mar::mar_grid_ok(G);
}

// the argument checks of all forms, and the tables.  bounds (null: the call has none): per segment lo[d], then hi[d]; they are checked
// last, and then the blocks are the wider ones
int mar_tables(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t G, double scale, MarTables& T)
{
    int rc = sum_front_args("param marginals", segs && probs, nseg);
    if (rc != MCE_OK) return rc;
    if (np < 1 || np > mce_mar::kMarMaxP) return fail(MCE_ERR_INVALID, "param marginals: %d probabilities (1 .. %d expected)", np, mce_mar::kMarMaxP);
    for (int32_t t = 0; t < np; ++t)
        if (!(probs[t] > 0.0 && probs[t] < 1.0)) return fail(MCE_ERR_INVALID, "param marginals: probability %d is %g (0 < p < 1 expected)", t, probs[t]);
    if (!mce_mar::mar_grid_ok(G)) return fail(MCE_ERR_INVALID, "param marginals: grid=%d (64, 128, 256, 512 or 1024 expected)", G);
    if (!mce_mar::mar_pos_finite(scale)) return fail(MCE_ERR_INVALID, "param marginals: scale=%g (finite and > 0 expected)", scale);
    rc = sum_front_tables("param marginals", segs, nseg, T, SumFrontNoCheck{}, [&](int32_t, const mce_summary_seg& g) {
        T.msegs.push_back(mce::MarSeg{T.parts, T.out_doubles});
        const int nparts = mce_mar::mar_nparts(g.n);
        T.parts += (int64_t)nparts * g.d;
        T.max_parts = std::max(T.max_parts, (int32_t)nparts);
        return mar_block_doubles(bounds != nullptr, g.d, np, G);
    });
    if (rc != MCE_OK) return rc;
    if (!bounds) return MCE_OK;
    for (int32_t s = 0; s < nseg; ++s) {
        const int32_t d = segs[s].d;
        for (int32_t j = 0; j < d; ++j) {
            const double L = bounds[j], U = bounds[d + j];
            if (!mce_marb::marb_bounds_ok(L, U))
                return fail(MCE_ERR_INVALID, "param marginals: segment %d, column %d has the bounds (%g, %g) (lo < hi, neither NaN expected)", s, j, L, U);
            T.bnd.push_back(L);
            T.bnd.push_back(U);
        }
        bounds += 2 * (size_t)d;
    }
    return MCE_OK;
}

// the _dev form of both families
template <bool kBounds>
int mar_dev(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale, double* out, void* ws,
            size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out || (kBounds && !bounds)) return fail(MCE_ERR_INVALID, "null pointer argument");
    MarTables T;
    int rc = mar_tables(segs, nseg, bounds, probs, np, grid, scale, T);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const MarWs W(kBounds, T.tiles.nrows, nseg, T.dmax, np, grid, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param marginals", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    if ((size_t)T.parts > mar_max_parts(T.tiles.nrows, nseg) * (size_t)T.dmax) return fail(MCE_ERR_WORKSPACE, "param marginals: %lld parts, fewer planned", (long long)T.parts);
    const int G = grid, nblk = mce_mar::mar_nblocks(G);
    const int64_t R = (int64_t)T.runs.size();
    if (R * nblk > mce_seg::kSegMaxTiles) return fail(MCE_ERR_INVALID, "param marginals: %lld columns in one call", (long long)R);
    MCE_HIP(hipMemcpyAsync(W.msegs, T.msegs.data(), T.msegs.size() * sizeof(MarSeg), hipMemcpyHostToDevice, st));
    if (kBounds) MCE_HIP(hipMemcpyAsync(W.bnd, T.bnd.data(), T.bnd.size() * 8, hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.probs, probs, (size_t)np * 8, hipMemcpyHostToDevice, st));
    // the moments, by summary's kernels as they stand
    if ((rc = sum_front_launch(W, T, nseg, true, st)) != MCE_OK) return rc;
    // the bandwidths and grids (and end flags); the kernel sums per part; the fold (and the boundary kernel); the decisions; the blocks
    const dim3 mt(kMarThreads);
    hipLaunchKernelGGL(mar_prep_kernel<kBounds>, dim3((unsigned)((R + kMarThreads - 1) / kMarThreads)), mt, 0, st, W.segs, W.runs, R, W.sys, W.col, W.bnd, G, scale, W.prm);
    if (T.max_parts > 0)
        hipLaunchKernelGGL(mar_density_kernel<kBounds>, dim3((unsigned)(R * nblk), (unsigned)T.max_parts), mt, 0, st, W.segs, W.msegs, W.runs, W.prm, G, nblk, W.S);
    hipLaunchKernelGGL(mar_fold_kernel<kBounds>, dim3((unsigned)(R * nblk)), mt, 0, st, W.segs, W.msegs, W.runs, W.prm, W.sys, G, nblk, (int)np, W.S, W.res);
    hipLaunchKernelGGL(mar_hpd_kernel<kBounds>, dim3((unsigned)R), mt, 0, st, W.segs, W.msegs, W.runs, W.prm, W.probs, (int)np, G, W.res);
    hipLaunchKernelGGL(mar_result_kernel<kBounds>, dim3((unsigned)nseg), mt, 0, st, W.segs, W.msegs, W.sys, W.col, W.prm, G, (int)np, W.res);
    return seg_dev_end(out, W.res, (size_t)T.out_doubles, st);
}

// the _f64 form of both families
template <bool kBounds>
int mar_f64(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale, double* out, int32_t device)
{
    if (!out || (kBounds && !bounds)) return fail(MCE_ERR_INVALID, "null pointer argument");
    MarTables T;
    int rc = mar_tables(segs, nseg, bounds, probs, np, grid, scale, T);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    SegStage data;
    DevBuf ws;
    std::vector<mce_summary_seg> dsegs;
    if ((rc = seg_stage_xw(segs, nseg, data, dsegs)) != MCE_OK) return rc;
    for (mce_summary_seg& g : dsegs) g.fs = nullptr;             // (the likelihood column is not an input)
    const size_t wsb = MarWs(kBounds, T.tiles.nrows, nseg, T.dmax, np, grid).total;
    MCE_HIP(ws.alloc(wsb));
    return mar_dev<kBounds>(dsegs.data(), nseg, bounds, probs, np, grid, scale, out, ws.p, wsb, nullptr);
}

}  // namespace

extern "C" {

size_t mce_param_marginals_out_doubles(int32_t d, int32_t np, int32_t grid) { return mar_shape_ok(1, d, np, grid) ? (size_t)mar_block_doubles(false, d, np, grid) : 0; }
size_t mce_param_marginals_bounded_out_doubles(int32_t d, int32_t np, int32_t grid) { return mar_shape_ok(1, d, np, grid) ? (size_t)mar_block_doubles(true, d, np, grid) : 0; }

size_t mce_param_marginals_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t grid)
{
    if (nrows_total < 0 || !mar_shape_ok(nseg, dmax, np, grid)) return 0;
    return MarWs(false, nrows_total, nseg, dmax, np, grid).total;
}
size_t mce_param_marginals_bounded_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t grid)
{
    if (nrows_total < 0 || !mar_shape_ok(nseg, dmax, np, grid)) return 0;
    return MarWs(true, nrows_total, nseg, dmax, np, grid).total;
}

int mce_param_marginals_dev(const mce_summary_seg* segs, int32_t nseg, const double* probs, int32_t np, int32_t grid, double scale, double* out, void* ws,
                            size_t ws_bytes, void* stream)
{
    return mar_dev<false>(segs, nseg, nullptr, probs, np, grid, scale, out, ws, ws_bytes, stream);
}
int mce_param_marginals_bounded_dev(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
                                    double* out, void* ws, size_t ws_bytes, void* stream)
{
    return mar_dev<true>(segs, nseg, bounds, probs, np, grid, scale, out, ws, ws_bytes, stream);
}

int mce_param_marginals_f64(const mce_summary_seg* segs, int32_t nseg, const double* probs, int32_t np, int32_t grid, double scale, double* out, int32_t device)
{
    return mar_f64<false>(segs, nseg, nullptr, probs, np, grid, scale, out, device);
}
int mce_param_marginals_bounded_f64(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
                                    double* out, int32_t device)
{
    return mar_f64<true>(segs, nseg, bounds, probs, np, grid, scale, out, device);
}

}  // extern "C"
