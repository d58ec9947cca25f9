// capi_sum_front.hpp -- part of capi.hip (one translation unit): the front that the _dev forms of capi_summary.hpp, capi_cov.hpp,
// capi_marginals.hpp and capi_contours.hpp share, which is summary's weighted moments (sum_tile / sum_sys / sum_col and, but for cov,
// sum_var_tile / sum_var_col of param_summary_kernels.hpp): the head of their workspaces, the per-segment checks and tables, and the
// launches.  Each family keeps its own argument checks; the error texts differ in their prefix (`who`) alone.
#pragma once

#include "capi_seg.hpp"
#include "param_summary_kernels.hpp"

namespace {

constexpr int32_t kSumMaxSegs = 1 << 16;
constexpr int64_t kSumMaxRows = 0x7fffffffLL;                   // (rocPRIM's segmented sort counts a pass in 32 bits)

// the head of a workspace: nrows_total rows in nseg segments, at most dmax columns.  with_var = false (cov): no second pass, no `part`
struct SumFrontWs {
    mce::SumSeg* segs;
    int64_t* tile0;
    double *head, *cols, *part, *sys, *col;
    mce::SumRun* runs;
    void take(WsPlan& P, int64_t nrows_total, int32_t nseg, int32_t dmax, bool with_var)
    {
        const size_t S = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows_total, nseg), D = (size_t)dmax, R = S * D;
        segs = P.take<mce::SumSeg>(S);
        tile0 = P.take<int64_t>(S);
        head = P.take<double>(T * mce::kSumTileHead);
        cols = P.take<double>(T * mce::kSumTileCol * D);
        part = with_var ? P.take<double>(T * D) : nullptr;
        sys = P.take<double>(S * mce::kSumSys);
        col = P.take<double>(R * mce::kSumCol);
        runs = P.take<mce::SumRun>(R);
    }
};

struct SumFrontTables {
    std::vector<mce::SumSeg> segs;
    mce_seg::SegTable tiles;
    std::vector<mce::SumRun> runs;                              // one per (system, column), in that order
    int64_t out_doubles = 0;
    int32_t dmax = 1;
};

// the first two checks of every family (ptrs: none of its pointer arguments is null); its own argument checks follow them
int sum_front_args(const char* who, bool ptrs, int32_t nseg)
{
    if (!ptrs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kSumMaxSegs) return fail(MCE_ERR_INVALID, "%s: %d segments (1 .. %d expected)", who, nseg, kSumMaxSegs);
    return MCE_OK;
}

// the per-segment checks and the tables.  between(s, g): MCE_OK, or the family's own refusal of segment s, which comes after the
// check of d and before that of the rows; block(s, g): the doubles of the segment's result block (T.out_doubles is still its offset),
// and the family's own counting.  fs stays null: summary sets its own
template <class Seg, class Between, class Block>
int sum_front_tables(const char* who, const Seg* segs, int32_t nseg, SumFrontTables& T, Between between, Block block)
{
    T.segs.assign((size_t)nseg, mce::SumSeg{});
    for (int32_t s = 0; s < nseg; ++s) {
        const Seg& g = segs[s];
        if (g.d < 1 || g.d > mce_sum::kSumMaxDim) return fail(MCE_ERR_INVALID, "%s: segment %d has d=%d (1 .. %d expected)", who, s, g.d, mce_sum::kSumMaxDim);
        const int rc = between(s, g);
        if (rc != MCE_OK) return rc;
        if (g.n < 0 || g.n > kSumMaxRows || g.ld < g.d || (g.n > 0 && (!g.x || !g.w)))
            return fail(MCE_ERR_INVALID, "%s: segment %d has %lld rows, ld=%lld, d=%d at x %s, w %s", who, s, (long long)g.n, (long long)g.ld, g.d,
                        g.x ? "valid" : "null", g.w ? "valid" : "null");
        mce::SumSeg& o = T.segs[(size_t)s];
        o.x = g.x; o.w = g.w; o.fs = nullptr; o.ld = g.ld; o.n = g.n; o.d = g.d; o.pad = 0;
        o.out_off = T.out_doubles;
        o.col0 = (int64_t)T.runs.size();
        T.out_doubles += block(s, g);
        T.tiles.add(g.n);
        T.dmax = std::max(T.dmax, g.d);
        for (int32_t j = 0; j < g.d; ++j) T.runs.push_back(mce::SumRun{0, 0, s, j});
    }
    if (!T.tiles.fits()) return fail(MCE_ERR_INVALID, "%s: %lld rows in one call", who, (long long)T.tiles.nrows);
    return MCE_OK;
}

struct SumFrontNoCheck {
    template <class Seg> int operator()(int32_t, const Seg&) const { return MCE_OK; }
};

// after seg_dev_begin: the runs, then the moments of every (system, column): W, A2, the used rows, the refusals, m, min, max and, with_var,
// the centred second pass: v
int sum_front_launch(const SumFrontWs& W, const SumFrontTables& T, int32_t nseg, bool with_var, hipStream_t st)
{
    using namespace mce;
    MCE_HIP(hipMemcpyAsync(W.runs, T.runs.data(), T.runs.size() * sizeof(SumRun), hipMemcpyHostToDevice, st));
    const dim3 tb(kPsumThreads), per_tile((unsigned)T.tiles.ntiles), per_run((unsigned)T.runs.size());
    const int dmax = T.dmax;
    if (T.tiles.ntiles > 0) hipLaunchKernelGGL(sum_tile_kernel, per_tile, tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.head, W.cols);
    hipLaunchKernelGGL(sum_sys_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.head, W.sys);
    hipLaunchKernelGGL(sum_col_kernel, per_run, tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.cols, W.sys, W.col);
    if (!with_var) return MCE_OK;
    if (T.tiles.ntiles > 0) hipLaunchKernelGGL(sum_var_tile_kernel, per_tile, tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.col, W.part);
    hipLaunchKernelGGL(sum_var_col_kernel, per_run, tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.part, W.sys, W.col);
    return MCE_OK;
}

}  // namespace
