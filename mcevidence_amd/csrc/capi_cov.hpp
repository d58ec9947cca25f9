// capi_cov.hpp -- part of capi.hip (one translation unit): mce_param_cov_out_doubles / mce_param_cov_workspace_bytes /
// mce_param_cov_dev / mce_param_cov_f64: the weighted mean and covariance matrix of the parameter columns of MANY systems (the ready
// roots of a farm wave) that are on the device, in one call (param_cov_kernels.hpp has the launches, param_cov.hpp the rule).
// Everything is enqueued on the caller's stream; the host waits once, for one block of results.  Argument checks come before any device
// call.  Six launches, whatever the number of systems.
#pragma once

#include "capi_seg.hpp"
#include "param_cov.hpp"
#include "param_cov_kernels.hpp"

namespace {

constexpr int32_t kCovMaxSegs = 1 << 16;
constexpr int64_t kCovMaxRows = 0x7fffffffLL;

// the workspace of a call: nrows_total rows in nseg segments, at most dmax columns
struct CovWs {
    mce::SumSeg* segs;
    int64_t* tile0;
    double *head, *cols, *sys, *col, *gram, *res;
    mce::SumRun* runs;
    size_t total;
    CovWs(int64_t nrows_total, int32_t nseg, int32_t dmax, void* ws = nullptr)
    {
        const size_t S = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows_total, nseg), R = S * (size_t)dmax, D = (size_t)dmax;
        WsPlan P(ws);
        segs = P.take<mce::SumSeg>(S);
        tile0 = P.take<int64_t>(S);
        head = P.take<double>(T * mce::kSumTileHead);
        cols = P.take<double>(T * mce::kSumTileCol * D);
        sys = P.take<double>(S * mce::kSumSys);
        col = P.take<double>(R * mce::kSumCol);
        runs = P.take<mce::SumRun>(R);
        gram = P.take<double>(T * (size_t)mce_cov::cov_nblocks(dmax) * mce::kPcovBlockDoubles);
        res = P.take<double>(S * (size_t)mce_cov::cov_out_doubles(dmax));
        total = P.total;
    }
};

struct CovTables {
    std::vector<mce::SumSeg> segs;
    mce_seg::SegTable tiles;
    std::vector<mce::SumRun> runs;
    int64_t out_doubles = 0;
    int32_t dmax = 1;
};

// the argument checks of both forms, and the tables
int cov_tables(const mce_cov_seg* segs, int32_t nseg, CovTables& T)
{
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kCovMaxSegs) return fail(MCE_ERR_INVALID, "param cov: %d segments (1 .. %d expected)", nseg, kCovMaxSegs);
    T.segs.assign((size_t)nseg, mce::SumSeg{});
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_cov_seg& g = segs[s];
        if (g.d < 1 || g.d > mce_cov::kCovMaxDim) return fail(MCE_ERR_INVALID, "param cov: segment %d has d=%d (1 .. %d expected)", s, g.d, mce_cov::kCovMaxDim);
        if (g.n < 0 || g.n > kCovMaxRows || g.ld < g.d || (g.n > 0 && (!g.x || !g.w)))
            return fail(MCE_ERR_INVALID, "param cov: segment %d has %lld rows, ld=%lld, d=%d at x %s, w %s", s, (long long)g.n, (long long)g.ld, g.d,
                        g.x ? "valid" : "null", g.w ? "valid" : "null");
        mce::SumSeg& o = T.segs[(size_t)s];
        o.x = g.x; o.w = g.w; o.fs = nullptr; o.ld = g.ld; o.n = g.n; o.d = g.d; o.pad = 0;
        o.out_off = T.out_doubles;
        o.col0 = (int64_t)T.runs.size();
        T.out_doubles += mce_cov::cov_out_doubles(g.d);
        T.tiles.add(g.n);
        T.dmax = std::max(T.dmax, g.d);
        for (int32_t j = 0; j < g.d; ++j) T.runs.push_back(mce::SumRun{0, 0, s, j});
    }
    if (!T.tiles.fits()) return fail(MCE_ERR_INVALID, "param cov: %lld rows in one call", (long long)T.tiles.nrows);
    return MCE_OK;
}

// the Gram pass stages more LDS than the default limit: raise it once per device (a failure is not remembered: the next call asks again)
int cov_attr_once()
{
    static std::atomic<bool> attr_set[kMaxDevices];
    int dev = 0;
    MCE_HIP(hipGetDevice(&dev));
    if (dev >= kMaxDevices || !attr_set[dev].load()) {
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::cov_gram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mce::cov_gram_lds_bytes()));
        if (dev < kMaxDevices) attr_set[dev].store(true);
    }
    return MCE_OK;
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
    if (nrows_total < 0 || nseg < 1 || nseg > kCovMaxSegs || dmax < 1 || dmax > mce_cov::kCovMaxDim) return 0;
    return CovWs(nrows_total, nseg, dmax).total;
}

int mce_param_cov_dev(const mce_cov_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    CovTables T;
    int rc = cov_tables(segs, nseg, T);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const CovWs W(T.tiles.nrows, nseg, T.dmax, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param cov", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    if ((rc = cov_attr_once()) != MCE_OK) return rc;
    const int dmax = T.dmax, nblkmax = mce_cov::cov_nblocks(dmax);
    const int64_t R = (int64_t)T.runs.size();
    MCE_HIP(hipMemcpyAsync(W.runs, T.runs.data(), T.runs.size() * sizeof(SumRun), hipMemcpyHostToDevice, st));
    const dim3 tb(kPsumThreads);
    const unsigned ntiles = (unsigned)T.tiles.ntiles;
    // pass 1: W, A2, the used rows, the refusals and the means, by summary's kernels as they stand
    if (ntiles > 0) hipLaunchKernelGGL(sum_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.head, W.cols);
    hipLaunchKernelGGL(sum_sys_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.head, W.sys);
    hipLaunchKernelGGL(sum_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.cols, W.sys, W.col);
    // pass 2: the centred Gram matrix of every tile; pass 3: the fold; pass 4: the result
    if (ntiles > 0) hipLaunchKernelGGL(cov_gram_kernel, dim3(ntiles), dim3(kPcovThreads), cov_gram_lds_bytes(), st, W.segs, W.tile0, (int)nseg, nblkmax, W.col, W.gram);
    hipLaunchKernelGGL(cov_fold_kernel, dim3((unsigned)((int64_t)nseg * nblkmax)), dim3(kPcovThreads), 0, st, W.segs, W.tile0, nblkmax, W.gram, W.sys, W.res);
    hipLaunchKernelGGL(cov_result_kernel, dim3((unsigned)nseg), dim3(kPcovThreads), 0, st, W.segs, W.sys, W.col, W.res);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, W.res, (size_t)T.out_doubles * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    return MCE_OK;
}

int mce_param_cov_f64(const mce_cov_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    CovTables T;
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
