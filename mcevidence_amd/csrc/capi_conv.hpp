// capi_conv.hpp -- part of capi.hip (one translation unit): mce_chain_conv_workspace_bytes / mce_chain_conv_dev / mce_chain_conv_f64:
// the Gelman-Rubin R-1 of the burned chains of MANY systems (the roots of a farm wave) that are on the device, in one call
// (chain_conv_kernels.hpp has the passes, chain_conv.hpp the rule, capi_eig.hpp the solver that is launched twice).  Everything is
// enqueued on the caller's stream; the host waits once, for one block of results.  Argument checks come before any device call.
#pragma once

#include "chain_conv.hpp"
#include "chain_conv_kernels.hpp"

namespace {

// the workspace of a call: nrows rows in nseg segments of nsys systems, ndim columns
struct ConvWs {
    mce::ConvSeg* segs;
    mce::ConvSys* sys;
    double *tiles, *seg1, *seg2, *centre, *partial, *Cs, *Wn, *dn, *v, *evec, *scale, *lam, *T, *pp, *res;
    int32_t *tbad, *segbad, *stat1, *stat2, *status, *used, *pd;
    size_t total;
    ConvWs(int64_t nrows, int32_t nseg, int32_t nsys, int32_t ndim, void* ws = nullptr)
    {
        const size_t max_tiles = (size_t)(nrows / mce::kConvTileRows + nseg);
        const size_t nc = (size_t)ndim + 1, npair = (size_t)mce_conv::conv_npair(ndim), dd = (size_t)ndim * ndim, S = (size_t)nseg, Y = (size_t)nsys;
        WsPlan P(ws);
        segs = P.take<mce::ConvSeg>(S);
        sys = P.take<mce::ConvSys>(Y);
        tiles = P.take<double>(max_tiles * nc);
        tbad = P.take<int32_t>(max_tiles * nc);
        seg1 = P.take<double>(S * nc);
        segbad = P.take<int32_t>(S * nc);
        seg2 = P.take<double>(S * nc);
        centre = P.take<double>(Y * ndim);
        partial = P.take<double>(max_tiles * npair);
        Cs = P.take<double>(S * npair);
        Wn = P.take<double>(Y * dd);
        dn = P.take<double>(S * ndim);
        v = P.take<double>(S * ndim);
        evec = P.take<double>(Y * dd);
        scale = P.take<double>(Y * ndim);
        lam = P.take<double>(Y * ndim);
        stat1 = P.take<int32_t>(Y * mce_eig::kStatInts);
        stat2 = P.take<int32_t>(Y * mce_eig::kStatInts);
        T = P.take<double>(Y * dd);
        pp = P.take<double>(Y * ndim);
        status = P.take<int32_t>(Y * 2);
        used = P.take<int32_t>(Y);
        pd = P.take<int32_t>(Y);
        res = P.take<double>(Y * ((size_t)ndim + 4));
        total = P.total;
    }
};

// the argument checks of both forms, and the tables: seg_sys non-decreasing in 0 .. nsys - 1, at most MCE_CONV_MAX_SEGMENTS segments
// and at least two with rows per system
int conv_tables(const mce_chain_part* segs, const int32_t* seg_sys, int32_t nseg, int32_t nsys, int64_t ncols, int32_t iw, int32_t itheta, int32_t ndim,
                std::vector<mce::ConvSeg>& table, std::vector<mce::ConvSys>& systems, int64_t& nrows, int64_t& ntiles)
{
    if (!segs || !seg_sys) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (ndim < 1 || ndim > mce_conv::kConvMaxDim) return fail(MCE_ERR_INVALID, "chain conv: ndim=%d (1 .. %d expected)", ndim, mce_conv::kConvMaxDim);
    if (ncols < 1 || ncols > (1 << 20)) return fail(MCE_ERR_INVALID, "chain conv: ncols=%lld", (long long)ncols);
    if (iw < 0 || iw >= ncols || itheta < 0 || itheta >= ncols || ndim > ncols - itheta)
        return fail(MCE_ERR_INVALID, "chain conv: columns iw=%d itheta=%d ndim=%d of %lld", iw, itheta, ndim, (long long)ncols);
    if (nsys < 1 || nseg < 1 || nsys > (1 << 20) || nseg > (1 << 24)) return fail(MCE_ERR_INVALID, "chain conv: %d segments in %d systems", nseg, nsys);
    table.assign((size_t)nseg, mce::ConvSeg());
    systems.assign((size_t)nsys, mce::ConvSys{0, 0});
    std::vector<int> with_rows((size_t)nsys, 0);
    nrows = 0;
    ntiles = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const int32_t y = seg_sys[s];
        if (y < 0 || y >= nsys || (s > 0 && y < seg_sys[s - 1]))
            return fail(MCE_ERR_INVALID, "chain conv: seg_sys[%d]=%d (non-decreasing values in 0 .. %d expected)", s, y, nsys - 1);
        const int rc = prep_check_part("chain conv", s, segs[s]);
        if (rc != MCE_OK) return rc;
        if (systems[(size_t)y].nseg == 0) systems[(size_t)y].seg0 = s;
        if (++systems[(size_t)y].nseg > MCE_CONV_MAX_SEGMENTS)
            return fail(MCE_ERR_INVALID, "chain conv: system %d has more than %d segments", y, MCE_CONV_MAX_SEGMENTS);
        with_rows[(size_t)y] += segs[s].nrows > 0 ? 1 : 0;
        mce::ConvSeg& q = table[(size_t)s];
        q.rows = segs[s].rows;
        q.nrows = segs[s].nrows;
        q.tile0 = ntiles;
        q.sys = y;
        q.pad = 0;
        ntiles += (q.nrows + mce::kConvTileRows - 1) / mce::kConvTileRows;
        nrows += q.nrows;
    }
    for (int32_t y = 0; y < nsys; ++y)
        if (with_rows[(size_t)y] < 2)
            return fail(MCE_ERR_INVALID, "chain conv: system %d has %d segments with rows (2 needed: measure by halves, or give more rows)", y,
                        with_rows[(size_t)y]);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_chain_conv_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t nsys, int32_t ndim)
{
    if (nrows_total < 0 || nseg < 1 || nsys < 1 || nsys > (1 << 20) || nseg > (1 << 24) || ndim < 1 || ndim > mce_conv::kConvMaxDim) return 0;
    return ConvWs(nrows_total, nseg, nsys, ndim).total;
}

int mce_chain_conv_dev(const mce_chain_part* segs, const int32_t* seg_sys, int32_t nseg, int32_t nsys, int64_t ncols, int32_t iw, int32_t itheta,
                       int32_t ndim, double* r_minus_1, double* per_param, int32_t* status, int32_t* nseg_used, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!r_minus_1 || !per_param || !status || !nseg_used) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<ConvSeg> table;
    std::vector<ConvSys> systems;
    int64_t nrows = 0, ntiles = 0;
    int rc = conv_tables(segs, seg_sys, nseg, nsys, ncols, iw, itheta, ndim, table, systems, nrows, ntiles);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    const ConvWs W(nrows, nseg, nsys, ndim, ws);
    if (ws_bytes < W.total) return fail(MCE_ERR_WORKSPACE, "chain conv: workspace of %zu bytes, %zu needed", ws_bytes, W.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    MCE_HIP(hipMemcpyAsync(W.segs, table.data(), table.size() * sizeof(ConvSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.sys, systems.data(), systems.size() * sizeof(ConvSys), hipMemcpyHostToDevice, st));
    const int nc = ndim + 1, npair = mce_conv::conv_npair(ndim);
    int cl = 1;
    while (cl < nc) cl <<= 1;
    auto grid = [](int64_t work) { return dim3((unsigned)((work + kConvThreads - 1) / kConvThreads)); };
    const dim3 tb(kConvThreads);
    // steps 1, 2: the sums, the centre, the sums about the centre
    hipLaunchKernelGGL(conv_sum_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, W.segs, (int)nseg, ncols, (int)iw, (int)itheta, (int)ndim, cl,
                       (const double*)nullptr, W.tiles, W.tbad);
    hipLaunchKernelGGL(conv_sum_final_kernel, grid((int64_t)nseg * nc), tb, 0, st, W.segs, (int)nseg, (int)ndim, W.tiles, W.tbad, W.seg1, W.segbad);
    hipLaunchKernelGGL(conv_centre_kernel, grid((int64_t)nsys * ndim), tb, 0, st, W.sys, (int)nsys, (int)ndim, W.seg1, W.centre);
    hipLaunchKernelGGL(conv_sum_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, W.segs, (int)nseg, ncols, (int)iw, (int)itheta, (int)ndim, cl, W.centre, W.tiles,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(conv_sum_final_kernel, grid((int64_t)nseg * nc), tb, 0, st, W.segs, (int)nseg, (int)ndim, W.tiles, (const int32_t*)nullptr, W.seg2,
                       (int32_t*)nullptr);
    // step 4
    const int nbd = (ndim + kConvBlock - 1) / kConvBlock, nblk = nbd * (nbd + 1) / 2;
    hipLaunchKernelGGL(conv_moment_kernel, dim3((unsigned)ntiles, (unsigned)((nblk + kConvThreads - 1) / kConvThreads)), tb, 0, st, W.segs, (int)nseg, ncols, (int)iw,
                       (int)itheta, (int)ndim, W.centre, W.seg1, W.seg2, W.partial);
    hipLaunchKernelGGL(conv_moment_final_kernel, grid((int64_t)nseg * npair), tb, 0, st, W.segs, (int)nseg, (int)ndim, W.seg1, W.partial, W.Cs);
    // steps 3, 5, 6, 7
    hipLaunchKernelGGL(conv_system_kernel, dim3((unsigned)nsys), tb, 0, st, W.segs, W.sys, (int)ndim, W.seg1, W.segbad, W.seg2, W.Cs, W.Wn, W.dn, W.pp, W.status,
                       W.used);
    MCE_HIP(hipGetLastError());
    if ((rc = launch_eig(W.Wn, ndim, nsys, W.evec, W.scale, W.lam, W.stat1, st)) != MCE_OK) return rc;
    // step 8
    hipLaunchKernelGGL(conv_t_kernel, dim3((unsigned)nsys), tb, 0, st, W.sys, (int)ndim, W.dn, W.evec, W.scale, W.lam, W.stat1, W.used, W.v, W.T, W.pd);
    MCE_HIP(hipGetLastError());
    if ((rc = launch_eig(W.T, ndim, nsys, W.evec, W.scale, W.lam, W.stat2, st)) != MCE_OK) return rc;
    hipLaunchKernelGGL(conv_result_kernel, grid((int64_t)nsys * (ndim + 4)), tb, 0, st, (int)nsys, (int)ndim, W.lam, W.stat1, W.pd, W.stat2, W.status, W.used, W.pp,
                       W.res);
    MCE_HIP(hipGetLastError());
    std::vector<double> res((size_t)nsys * (ndim + 4));
    MCE_HIP(hipMemcpyAsync(res.data(), W.res, res.size() * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    for (int32_t y = 0; y < nsys; ++y) {
        const double* r = res.data() + (size_t)y * (ndim + 4);
        r_minus_1[y] = r[0];
        status[2 * y] = (int32_t)r[1];
        status[2 * y + 1] = (int32_t)r[2];
        nseg_used[y] = (int32_t)r[3];
        for (int32_t j = 0; j < ndim; ++j) per_param[(size_t)y * ndim + j] = r[4 + j];
    }
    return MCE_OK;
}

int mce_chain_conv_f64(const mce_chain_part* segs, const int32_t* seg_sys, int32_t nseg, int32_t nsys, int64_t ncols, int32_t iw, int32_t itheta,
                       int32_t ndim, double* r_minus_1, double* per_param, int32_t* status, int32_t* nseg_used, int32_t device)
{
    if (!r_minus_1 || !per_param || !status || !nseg_used) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<mce::ConvSeg> table;
    std::vector<mce::ConvSys> systems;
    int64_t nrows = 0, ntiles = 0;
    int rc = conv_tables(segs, seg_sys, nseg, nsys, ncols, iw, itheta, ndim, table, systems, nrows, ntiles);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    DevBuf rows, ws;
    MCE_HIP(rows.alloc((size_t)std::max<int64_t>(nrows, 1) * ncols * sizeof(double)));
    std::vector<mce_chain_part> dsegs((size_t)nseg);
    int64_t at = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        dsegs[(size_t)s].rows = segs[s].nrows > 0 ? rows.as<double>() + at * ncols : nullptr;
        dsegs[(size_t)s].nrows = segs[s].nrows;
        if (segs[s].nrows > 0)
            MCE_HIP(hipMemcpy(rows.as<double>() + at * ncols, segs[s].rows, (size_t)segs[s].nrows * ncols * sizeof(double), hipMemcpyHostToDevice));
        at += segs[s].nrows;
    }
    const size_t wsb = mce_chain_conv_workspace_bytes(nrows, nseg, nsys, ndim);
    MCE_HIP(ws.alloc(wsb));
    return mce_chain_conv_dev(dsegs.data(), seg_sys, nseg, nsys, ncols, iw, itheta, ndim, r_minus_1, per_param, status, nseg_used, ws.p, wsb, nullptr);
}

}  // extern "C"
