// capi_cov.hpp -- part of capi.hip (one translation unit): mce_param_cov_out_doubles / mce_param_cov_workspace_bytes /
// mce_param_cov_dev / mce_param_cov_f64: the weighted mean and covariance matrix of the parameter columns of MANY systems (the ready
// roots of a farm wave) that are on the device, in one call (param_cov_kernels.hpp has the launches, param_cov.hpp the rule).
// Everything is enqueued on the caller's stream; the host waits once, for one block of results.  Argument checks come before any device
// call.  Six launches, whatever the number of systems: sum_tile / sum_sys / sum_col (capi_sum_front.hpp: the head of the workspace, the
// per-segment checks and tables and these launches, without the second pass), then cov_gram / cov_fold / cov_result.
#pragma once

#include "capi_sum_front.hpp"
#include "param_cov.hpp"
#include "param_cov_kernels.hpp"

namespace {

// the workspace of a call: nrows_total rows in nseg segments, at most dmax columns
struct CovWs : SumFrontWs {
    double *gram, *res;
    size_t total;
    CovWs(int64_t nrows_total, int32_t nseg, int32_t dmax, void* ws = nullptr)
    {
        WsPlan P(ws);
        take(P, nrows_total, nseg, dmax, false);
        gram = P.take<double>((size_t)mce_seg::seg_max_tiles(nrows_total, nseg) * (size_t)mce_cov::cov_nblocks(dmax) * mce::kPcovBlockDoubles);
        res = P.take<double>((size_t)nseg * (size_t)mce_cov::cov_out_doubles(dmax));
        total = P.total;
    }
};

// the argument checks of both forms, and the tables
int cov_tables(const mce_cov_seg* segs, int32_t nseg, SumFrontTables& T)
{
    const int rc = sum_front_args("param cov", segs != nullptr, nseg);
    if (rc != MCE_OK) return rc;
    return sum_front_tables("param cov", segs, nseg, T, SumFrontNoCheck{}, [](int32_t, const mce_cov_seg& g) { return mce_cov::cov_out_doubles(g.d); });
}

}  // namespace

extern "C" {

size_t mce_param_cov_out_doubles(int32_t d)
{
    if (d < 1 || d > mce_cov::kCovMaxDim) return 0;
    return (size_t)mce_cov::cov_out_doubles(d);
}

size_t mce_param_cov_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax)
{
    if (nrows_total < 0 || nseg < 1 || nseg > kSumMaxSegs || dmax < 1 || dmax > mce_cov::kCovMaxDim) return 0;
    return CovWs(nrows_total, nseg, dmax).total;
}

int mce_param_cov_dev(const mce_cov_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    SumFrontTables T;
    int rc = cov_tables(segs, nseg, T);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const CovWs W(T.tiles.nrows, nseg, T.dmax, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param cov", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    // the Gram pass stages more LDS than the default limit
    static std::atomic<bool> attr_set[kMaxDevices];
    if ((rc = seg_attr_once(attr_set, {{reinterpret_cast<const void*>(cov_gram_kernel), cov_gram_lds_bytes()}})) != MCE_OK) return rc;
    const int nblkmax = mce_cov::cov_nblocks(T.dmax);
    const unsigned ntiles = (unsigned)T.tiles.ntiles;
    // pass 1: W, A2, the used rows, the refusals and the means, by summary's kernels as they stand
    if ((rc = sum_front_launch(W, T, nseg, false, st)) != MCE_OK) return rc;
    // pass 2: the centred Gram matrix of every tile; pass 3: the fold; pass 4: the result
    if (ntiles > 0) hipLaunchKernelGGL(cov_gram_kernel, dim3(ntiles), dim3(kPcovThreads), cov_gram_lds_bytes(), st, W.segs, W.tile0, (int)nseg, nblkmax, W.col, W.gram);
    hipLaunchKernelGGL(cov_fold_kernel, dim3((unsigned)((int64_t)nseg * nblkmax)), dim3(kPcovThreads), 0, st, W.segs, W.tile0, nblkmax, W.gram, W.sys, W.res);
    hipLaunchKernelGGL(cov_result_kernel, dim3((unsigned)nseg), dim3(kPcovThreads), 0, st, W.segs, W.sys, W.col, W.res);
    return seg_dev_end(out, W.res, (size_t)T.out_doubles, st);
}

int mce_param_cov_f64(const mce_cov_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    SumFrontTables T;
    int rc = cov_tables(segs, nseg, T);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    SegStage data;
    DevBuf ws;
    std::vector<mce_cov_seg> dsegs;
    if ((rc = seg_stage_xw(segs, nseg, data, dsegs)) != MCE_OK) return rc;
    const size_t wsb = mce_param_cov_workspace_bytes(T.tiles.nrows, nseg, T.dmax);
    MCE_HIP(ws.alloc(wsb));
    return mce_param_cov_dev(dsegs.data(), nseg, out, ws.p, wsb, nullptr);
}

}  // extern "C"
