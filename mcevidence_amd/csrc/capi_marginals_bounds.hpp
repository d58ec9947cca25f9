// capi_marginals_bounds.hpp -- part of capi.hip (one translation unit): mce_param_marginals_bounded_out_doubles /
// mce_param_marginals_bounded_workspace_bytes / mce_param_marginals_bounded_dev / mce_param_marginals_bounded_f64: the 1-D marginal
// densities of capi_marginals.hpp for parameters with hard prior bounds (param_marginals_bounds_kernels.hpp has the launches,
// param_marginals_bounds.hpp the rule).  The bounds are a HOST array that travels with the segment table.  Everything is enqueued on
// the caller's stream; the host waits once, for one block of results.  Argument checks come before any device call.  Ten launches,
// whatever the number of systems.
#pragma once

#include "capi_marginals.hpp"
#include "param_marginals_bounds.hpp"
#include "param_marginals_bounds_kernels.hpp"

namespace {

// the workspace of a call: capi_marginals.hpp's MarWs with two sums per part, the bounds and the wider blocks
struct MarbWs {
    mce::SumSeg* segs;
    int64_t* tile0;
    double *head, *cols, *part, *sys, *col, *prm, *bnd, *probs, *SR, *res;
    mce::SumRun* runs;
    mce::MarSeg* msegs;
    size_t total;
    MarbWs(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t G, void* ws = nullptr)
    {
        const size_t Sg = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows_total, nseg), R = Sg * (size_t)dmax, D = (size_t)dmax;
        WsPlan P(ws);
        segs = P.take<mce::SumSeg>(Sg);
        tile0 = P.take<int64_t>(Sg);
        head = P.take<double>(T * mce::kSumTileHead);
        cols = P.take<double>(T * mce::kSumTileCol * D);
        part = P.take<double>(T * D);
        sys = P.take<double>(Sg * mce::kSumSys);
        col = P.take<double>(R * mce::kSumCol);
        runs = P.take<mce::SumRun>(R);
        msegs = P.take<mce::MarSeg>(Sg);
        prm = P.take<double>(R * mce::kMarbPrm);
        bnd = P.take<double>(R * 2);
        probs = P.take<double>((size_t)mce_mar::kMarMaxP + 1);
        SR = P.take<double>(mar_max_parts(nrows_total, nseg) * D * 2 * (size_t)G);
        res = P.take<double>(Sg * (size_t)mce_marb::marb_out_doubles(dmax, np, G));
        total = P.total;
    }
};

// the argument checks of both forms and the tables: mar_tables', then the bounds per run (L, U) and the blocks' places
int marb_tables(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t G, double scale, MarTables& T,
                std::vector<double>& bnd)
{
    if (!bounds) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = mar_tables(segs, nseg, probs, np, G, scale, T);
    if (rc != MCE_OK) return rc;
    bnd.assign(T.runs.size() * 2, 0.0);
    const double* b = bounds;
    T.out_doubles = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const int32_t d = segs[s].d;
        for (int32_t j = 0; j < d; ++j) {
            const double L = b[j], U = b[d + j];
            if (!mce_marb::marb_bounds_ok(L, U))
                return fail(MCE_ERR_INVALID, "param marginals: segment %d, column %d has the bounds (%g, %g) (lo < hi, neither NaN expected)", s, j, L, U);
            const size_t r = (size_t)T.segs[(size_t)s].col0 + (size_t)j;
            bnd[2 * r] = L;
            bnd[2 * r + 1] = U;
        }
        b += 2 * (size_t)d;
        T.segs[(size_t)s].out_off = T.out_doubles;
        T.msegs[(size_t)s].out_off = T.out_doubles;
        T.out_doubles += mce_marb::marb_out_doubles(d, np, G);
    }
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_param_marginals_bounded_out_doubles(int32_t d, int32_t np, int32_t grid)
{
    if (!mar_shape_ok(1, d, np, grid)) return 0;
    return (size_t)mce_marb::marb_out_doubles(d, np, grid);
}

size_t mce_param_marginals_bounded_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax, int32_t np, int32_t grid)
{
    if (nrows_total < 0 || !mar_shape_ok(nseg, dmax, np, grid)) return 0;
    return MarbWs(nrows_total, nseg, dmax, np, grid).total;
}

int mce_param_marginals_bounded_dev(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
                                    double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    MarTables T;
    std::vector<double> bnd;
    int rc = marb_tables(segs, nseg, bounds, probs, np, grid, scale, T, bnd);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const MarbWs W(T.tiles.nrows, nseg, T.dmax, np, grid, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param marginals", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    if ((size_t)T.parts > mar_max_parts(T.tiles.nrows, nseg) * (size_t)T.dmax) return fail(MCE_ERR_WORKSPACE, "param marginals: %lld parts, fewer planned", (long long)T.parts);
    const int dmax = T.dmax, G = grid, nblk = mce_mar::mar_nblocks(G);
    const int64_t R = (int64_t)T.runs.size();
    if (R * nblk > mce_seg::kSegMaxTiles) return fail(MCE_ERR_INVALID, "param marginals: %lld columns in one call", (long long)R);
    MCE_HIP(hipMemcpyAsync(W.runs, T.runs.data(), T.runs.size() * sizeof(SumRun), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.msegs, T.msegs.data(), T.msegs.size() * sizeof(MarSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.bnd, bnd.data(), bnd.size() * 8, hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.probs, probs, (size_t)np * 8, hipMemcpyHostToDevice, st));
    const dim3 tb(kPsumThreads);
    const unsigned ntiles = (unsigned)T.tiles.ntiles;
    // the moments, by summary's kernels as they stand
    if (ntiles > 0) hipLaunchKernelGGL(sum_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.head, W.cols);
    hipLaunchKernelGGL(sum_sys_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.head, W.sys);
    hipLaunchKernelGGL(sum_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.cols, W.sys, W.col);
    if (ntiles > 0) hipLaunchKernelGGL(sum_var_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.col, W.part);
    hipLaunchKernelGGL(sum_var_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.part, W.sys, W.col);
    // the bandwidths, grids and end flags; the two kernel sums per part; the fold and the boundary kernel; the decisions; the blocks
    const dim3 mt(kMarThreads);
    hipLaunchKernelGGL(marb_prep_kernel, dim3((unsigned)((R + kMarThreads - 1) / kMarThreads)), mt, 0, st, W.segs, W.runs, R, W.sys, W.col, W.bnd, G, scale, W.prm);
    if (T.max_parts > 0)
        hipLaunchKernelGGL(marb_density_kernel, dim3((unsigned)(R * nblk), (unsigned)T.max_parts), mt, 0, st, W.segs, W.msegs, W.runs, W.prm, G, nblk, W.SR);
    hipLaunchKernelGGL(marb_fold_kernel, dim3((unsigned)(R * nblk)), mt, 0, st, W.segs, W.msegs, W.runs, W.prm, W.sys, G, nblk, (int)np, W.SR, W.res);
    hipLaunchKernelGGL(marb_hpd_kernel, dim3((unsigned)R), mt, 0, st, W.segs, W.msegs, W.runs, W.prm, W.probs, (int)np, G, W.res);
    hipLaunchKernelGGL(marb_result_kernel, dim3((unsigned)nseg), mt, 0, st, W.segs, W.msegs, W.sys, W.col, W.prm, G, (int)np, W.res);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, W.res, (size_t)T.out_doubles * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    return MCE_OK;
}

int mce_param_marginals_bounded_f64(const mce_summary_seg* segs, int32_t nseg, const double* bounds, const double* probs, int32_t np, int32_t grid, double scale,
                                    double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    MarTables T;
    std::vector<double> bnd;
    int rc = marb_tables(segs, nseg, bounds, probs, np, grid, scale, T, bnd);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    size_t elems = 0;
    for (int32_t s = 0; s < nseg; ++s) elems += (size_t)segs[s].n * ((size_t)segs[s].d + 1);
    SegStage data;
    DevBuf ws;
    if ((rc = data.alloc(elems * sizeof(double))) != MCE_OK) return rc;
    std::vector<mce_summary_seg> dsegs(segs, segs + nseg);
    for (mce_summary_seg& g : dsegs) {
        // the d measured columns, packed: ld = d on the device; the likelihood column is not an input
        if ((rc = data.put(g.x, (size_t)g.n, g.x, (size_t)g.d, (size_t)g.ld)) != MCE_OK || (rc = data.put(g.w, (size_t)g.n, g.w)) != MCE_OK) return rc;
        g.ld = g.d;
        g.fs = nullptr;
    }
    const size_t wsb = mce_param_marginals_bounded_workspace_bytes(T.tiles.nrows, nseg, T.dmax, np, grid);
    MCE_HIP(ws.alloc(wsb));
    return mce_param_marginals_bounded_dev(dsegs.data(), nseg, bounds, probs, np, grid, scale, out, ws.p, wsb, nullptr);
}

}  // extern "C"
