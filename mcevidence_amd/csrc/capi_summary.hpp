// capi_summary.hpp -- part of capi.hip (one translation unit): mce_param_summary_out_doubles / mce_param_summary_workspace_bytes /
// mce_param_summary_dev / mce_param_summary_f64: the posterior summary (weighted means, variances, extremes, weighted quantiles, best
// fit) of the parameter columns of MANY systems (the ready roots of a farm wave) that are on the device, in one call
// (param_summary_kernels.hpp has the launches, param_summary.hpp the rule).  Everything is enqueued on the caller's stream; the host
// waits once, for one block of results.  Argument checks come before any device call.  The runs (system, column) are sorted in PASSES
// of at most pass_elems elements, so the number of launches depends on the number of passes, not on the number of systems.
#pragma once

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "capi_seg.hpp"
#include "param_summary.hpp"
#include "param_summary_kernels.hpp"

namespace {

constexpr int32_t kSumMaxSegs = 1 << 16;
constexpr int64_t kSumMaxRows = 0x7fffffffLL;                   // (rocPRIM's segmented sort counts a pass in 32 bits)

int64_t sum_pass_elems(int64_t pass_elems) { return pass_elems > 0 ? pass_elems : (int64_t)MCE_SUMMARY_PASS_ELEMS; }

// what rocPRIM asks for a pass of `size` elements in `segments` runs; without a device to ask, an estimate (the buffers are the
// caller's double buffers, so the temporary holds the runs' indices only)
size_t sum_sort_tmp_bytes(int64_t size, int64_t segments)
{
    size_t need = 0;
    // (a size query reads no element; the addresses only say that both halves of the double buffers exist, so that the temporary is
    // not sized to hold a second copy of the keys and the weights)
    unsigned long long* const kk = reinterpret_cast<unsigned long long*>(sizeof(double));
    double* const vv = reinterpret_cast<double*>(sizeof(double));
    rocprim::double_buffer<unsigned long long> k(kk, kk);
    rocprim::double_buffer<double> v(vv, vv);
    int nd = 0;
    if (hipGetDeviceCount(&nd) == hipSuccess && nd > 0 &&
        rocprim::segmented_radix_sort_pairs(nullptr, need, k, v, (unsigned)size, (unsigned)segments, (const unsigned*)nullptr, (const unsigned*)nullptr, 0u, 64u) ==
            hipSuccess)
        return need + 256;
    (void)hipGetLastError();
    return (size_t)65536 + 32 * (size_t)segments;
}

// the workspace of a call: nrows_total rows in nseg segments, the longest of nrows_max rows, at most dmax columns, nq targets
struct SumWs {
    mce::SumSeg* segs;
    int64_t* tile0;
    double *head, *cols, *part, *sys, *col, *quant, *q;
    mce::SumRun* runs;
    unsigned *ob, *oe;
    double *tot, *res;
    unsigned long long* keys[2];
    double* wts[2];
    void* tmp;
    size_t tmp_bytes, total;
    int64_t cap, max_runs, max_scan;
    SumWs(int64_t nrows_total, int64_t nrows_max, int32_t nseg, int32_t dmax, int32_t nq, int64_t pass_elems, void* ws = nullptr)
    {
        // a pass holds at most pass_elems elements, or one run; never more than there are elements at all
        cap = std::max<int64_t>(std::max(std::min(sum_pass_elems(pass_elems), nrows_total * dmax), nrows_max), 1);
        max_runs = (int64_t)nseg * dmax;
        max_scan = cap / mce::kSumScanTile + max_runs + 1;
        const size_t S = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows_total, nseg), R = (size_t)max_runs, D = (size_t)dmax;
        WsPlan P(ws);
        segs = P.take<mce::SumSeg>(S);
        tile0 = P.take<int64_t>(S);
        head = P.take<double>(T * mce::kSumTileHead);
        cols = P.take<double>(T * mce::kSumTileCol * D);
        part = P.take<double>(T * D);
        sys = P.take<double>(S * mce::kSumSys);
        col = P.take<double>(R * mce::kSumCol);
        quant = P.take<double>(R * (size_t)nq);
        q = P.take<double>((size_t)MCE_SUMMARY_MAX_Q);
        runs = P.take<mce::SumRun>(R);
        ob = P.take<unsigned>(R);
        oe = P.take<unsigned>(R);
        tot = P.take<double>((size_t)max_scan);
        res = P.take<double>(S * (size_t)mce_sum::sum_out_doubles(dmax, nq));
        for (int k = 0; k < 2; ++k) keys[k] = P.take<unsigned long long>((size_t)cap);
        for (int k = 0; k < 2; ++k) wts[k] = P.take<double>((size_t)cap);
        tmp_bytes = prep_align(sum_sort_tmp_bytes(cap, max_runs));
        tmp = P.take_bytes<void>(tmp_bytes);
        total = P.total;
    }
};

bool sum_shape_ok(int32_t nseg, int32_t dmax, int32_t nq, int64_t pass_elems)
{
    return nseg >= 1 && nseg <= kSumMaxSegs && dmax >= 1 && dmax <= mce_sum::kSumMaxDim && nq >= 1 && nq <= MCE_SUMMARY_MAX_Q && pass_elems >= 0 &&
           pass_elems <= kSumMaxRows;
}

struct SumPass {
    int64_t run0 = 0, nruns = 0, total = 0, ntiles = 0;
};

struct SumTables {
    std::vector<mce::SumSeg> segs;
    mce_seg::SegTable tiles;
    std::vector<mce::SumRun> runs;
    std::vector<unsigned> ob, oe;
    std::vector<SumPass> passes;
    int64_t nmax = 0, out_doubles = 0;
    int32_t dmax = 1;
};

// the argument checks of both forms, and the tables
int sum_tables(const mce_summary_seg* segs, int32_t nseg, const double* q, int32_t nq, int64_t pass_elems, SumTables& T)
{
    if (!segs || !q) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kSumMaxSegs) return fail(MCE_ERR_INVALID, "param summary: %d segments (1 .. %d expected)", nseg, kSumMaxSegs);
    if (nq < 1 || nq > MCE_SUMMARY_MAX_Q) return fail(MCE_ERR_INVALID, "param summary: %d targets (1 .. %d expected)", nq, MCE_SUMMARY_MAX_Q);
    for (int32_t t = 0; t < nq; ++t)
        if (!(q[t] > 0.0 && q[t] < 1.0)) return fail(MCE_ERR_INVALID, "param summary: target %d is %g (0 < q < 1 expected)", t, q[t]);
    if (pass_elems < 0 || pass_elems > kSumMaxRows) return fail(MCE_ERR_INVALID, "param summary: pass_elems=%lld", (long long)pass_elems);
    const int64_t pe = sum_pass_elems(pass_elems);
    T.segs.assign((size_t)nseg, mce::SumSeg{});
    SumPass cur;
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_summary_seg& g = segs[s];
        if (g.d < 1 || g.d > mce_sum::kSumMaxDim) return fail(MCE_ERR_INVALID, "param summary: segment %d has d=%d (1 .. %d expected)", s, g.d, mce_sum::kSumMaxDim);
        if (g.n < 0 || g.n > kSumMaxRows || g.ld < g.d || (g.n > 0 && (!g.x || !g.w)))
            return fail(MCE_ERR_INVALID, "param summary: segment %d has %lld rows, ld=%lld, d=%d at x %s, w %s", s, (long long)g.n, (long long)g.ld, g.d,
                        g.x ? "valid" : "null", g.w ? "valid" : "null");
        mce::SumSeg& o = T.segs[(size_t)s];
        o.x = g.x; o.w = g.w; o.fs = g.n > 0 ? g.fs : nullptr; o.ld = g.ld; o.n = g.n; o.d = g.d; o.pad = 0;
        o.out_off = T.out_doubles;
        o.col0 = (int64_t)T.runs.size();
        T.out_doubles += mce_sum::sum_out_doubles(g.d, nq);
        T.tiles.add(g.n);
        T.nmax = std::max(T.nmax, g.n);
        T.dmax = std::max(T.dmax, g.d);
        for (int32_t j = 0; j < g.d; ++j) {
            // a pass: runs in (system, column) order while they fit; a run longer than pass_elems is a pass of its own
            if (cur.nruns > 0 && cur.total + g.n > pe) {
                T.passes.push_back(cur);
                cur = SumPass{(int64_t)T.runs.size(), 0, 0, 0};
            }
            T.runs.push_back(mce::SumRun{cur.total, cur.ntiles, s, j});
            T.ob.push_back((unsigned)cur.total);
            T.oe.push_back((unsigned)(cur.total + g.n));
            cur.nruns += 1;
            cur.total += g.n;
            cur.ntiles += (g.n + mce::kSumScanTile - 1) / mce::kSumScanTile;
        }
    }
    if (cur.nruns > 0) T.passes.push_back(cur);
    if (!T.tiles.fits()) return fail(MCE_ERR_INVALID, "param summary: %lld rows in one call", (long long)T.tiles.nrows);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_param_summary_out_doubles(int32_t d, int32_t nq)
{
    if (d < 1 || d > mce_sum::kSumMaxDim || nq < 1 || nq > MCE_SUMMARY_MAX_Q) return 0;
    return (size_t)mce_sum::sum_out_doubles(d, nq);
}

size_t mce_param_summary_workspace_bytes(int64_t nrows_total, int64_t nrows_max, int32_t nseg, int32_t dmax, int32_t nq, int64_t pass_elems)
{
    if (nrows_total < 0 || nrows_max < 0 || nrows_max > nrows_total || nrows_max > kSumMaxRows || !sum_shape_ok(nseg, dmax, nq, pass_elems)) return 0;
    return SumWs(nrows_total, nrows_max, nseg, dmax, nq, pass_elems).total;
}

int mce_param_summary_dev(const mce_summary_seg* segs, int32_t nseg, const double* q, int32_t nq, int64_t pass_elems, double* out, void* ws, size_t ws_bytes,
                          void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    SumTables T;
    int rc = sum_tables(segs, nseg, q, nq, pass_elems, T);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const SumWs W(T.tiles.nrows, T.nmax, nseg, T.dmax, nq, pass_elems, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("param summary", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    const int dmax = T.dmax;
    const int64_t R = (int64_t)T.runs.size();

    MCE_HIP(hipMemcpyAsync(W.runs, T.runs.data(), T.runs.size() * sizeof(SumRun), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.ob, T.ob.data(), T.ob.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.oe, T.oe.data(), T.oe.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.q, q, (size_t)nq * 8, hipMemcpyHostToDevice, st));
    const dim3 tb(kPsumThreads);
    const unsigned ntiles = (unsigned)T.tiles.ntiles;
    if (ntiles > 0) hipLaunchKernelGGL(sum_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.head, W.cols);
    hipLaunchKernelGGL(sum_sys_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.head, W.sys);
    hipLaunchKernelGGL(sum_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.cols, W.sys, W.col);
    if (ntiles > 0) hipLaunchKernelGGL(sum_var_tile_kernel, dim3(ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, dmax, W.col, W.part);
    hipLaunchKernelGGL(sum_var_col_kernel, dim3((unsigned)R), tb, 0, st, W.segs, W.tile0, W.runs, dmax, W.part, W.sys, W.col);
    MCE_HIP(hipGetLastError());
    for (const SumPass& P : T.passes) {
        if (P.total > W.cap || P.ntiles > W.max_scan) return fail(MCE_ERR_WORKSPACE, "param summary: a pass of %lld elements, %lld planned", (long long)P.total, (long long)W.cap);
        rocprim::double_buffer<unsigned long long> keys(W.keys[0], W.keys[1]);
        rocprim::double_buffer<double> wts(W.wts[0], W.wts[1]);
        const SumRun* p_runs = W.runs + P.run0;
        if (P.total > 0) {
            hipLaunchKernelGGL(sum_keys_kernel, dim3((unsigned)((P.total + kPsumThreads - 1) / kPsumThreads)), tb, 0, st, W.segs, p_runs, (int)P.nruns, P.total,
                               keys.current(), wts.current());
            size_t need = 0;
            MCE_HIP(rocprim::segmented_radix_sort_pairs(nullptr, need, keys, wts, (unsigned)P.total, (unsigned)P.nruns, W.ob + P.run0, W.oe + P.run0, 0u, 64u, st));
            if (need > W.tmp_bytes) return fail(MCE_ERR_WORKSPACE, "param summary: the sort asks for %zu bytes, %zu planned", need, W.tmp_bytes);
            need = W.tmp_bytes;
            MCE_HIP(rocprim::segmented_radix_sort_pairs(W.tmp, need, keys, wts, (unsigned)P.total, (unsigned)P.nruns, W.ob + P.run0,
                                                        W.oe + P.run0, 0u, 64u, st));
            hipLaunchKernelGGL(sum_scan_tile_kernel, dim3((unsigned)P.ntiles), tb, 0, st, W.segs, p_runs, (int)P.nruns, wts.current(), W.tot);
        }
        hipLaunchKernelGGL(sum_search_kernel, dim3((unsigned)P.nruns), dim3(64), 0, st, W.segs, p_runs, P.run0, W.q, (int)nq, W.sys, keys.current(), wts.current(),
                           W.tot, W.quant);
        MCE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(sum_result_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.sys, W.col, W.quant, (int)nq, W.res);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, W.res, (size_t)T.out_doubles * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    return MCE_OK;
}

int mce_param_summary_f64(const mce_summary_seg* segs, int32_t nseg, const double* q, int32_t nq, int64_t pass_elems, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    SumTables T;
    int rc = sum_tables(segs, nseg, q, nq, pass_elems, T);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    size_t elems = 0;
    for (int32_t s = 0; s < nseg; ++s) elems += (size_t)segs[s].n * ((size_t)segs[s].d + 2);
    SegStage data;
    DevBuf ws;
    if ((rc = data.alloc(elems * sizeof(double))) != MCE_OK) return rc;
    std::vector<mce_summary_seg> dsegs(segs, segs + nseg);
    for (mce_summary_seg& g : dsegs) {
        // the d measured columns, packed: ld = d on the device
        if ((rc = data.put(g.x, (size_t)g.n, g.x, (size_t)g.d, (size_t)g.ld)) != MCE_OK || (rc = data.put(g.w, (size_t)g.n, g.w)) != MCE_OK ||
            (rc = data.put(g.fs, (size_t)g.n, g.fs)) != MCE_OK)
            return rc;
        g.ld = g.d;
    }
    const size_t wsb = mce_param_summary_workspace_bytes(T.tiles.nrows, T.nmax, nseg, T.dmax, nq, pass_elems);
    MCE_HIP(ws.alloc(wsb));
    return mce_param_summary_dev(dsegs.data(), nseg, q, nq, pass_elems, out, ws.p, wsb, nullptr);
}

}  // extern "C"
