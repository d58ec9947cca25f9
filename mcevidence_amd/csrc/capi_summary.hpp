// capi_summary.hpp -- part of capi.hip (one translation unit): mce_param_summary_out_doubles / mce_param_summary_workspace_bytes /
// mce_param_summary_dev / mce_param_summary_f64: the posterior summary (weighted means, variances, extremes, weighted quantiles, best
// fit) of the parameter columns of MANY systems (the ready roots of a farm wave) that are on the device, in one call
// (param_summary_kernels.hpp has the launches, param_summary.hpp the rule).  The weighted moments -- the head of the workspace, the
// per-segment checks and tables, the first five launches -- are capi_sum_front.hpp's, which cov, marginals and contours begin with too;
// here: fs, the passes and the quantiles.  Everything is enqueued on the caller's stream; the host waits once, for one block of results
// (seg_dev_end).  Argument checks come before any device call.  The runs (system, column) are sorted in PASSES of at most pass_elems
// elements, so the number of launches depends on the number of passes, not on the number of systems.
#pragma once

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "capi_sum_front.hpp"
#include "param_summary.hpp"

namespace {

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
struct SumWs : SumFrontWs {
    double *quant, *q;
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
        const size_t S = (size_t)nseg, R = (size_t)max_runs;
        WsPlan P(ws);
        take(P, nrows_total, nseg, dmax, true);
        quant = P.take<double>(R * (size_t)nq);
        q = P.take<double>((size_t)MCE_SUMMARY_MAX_Q);
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

struct SumTables : SumFrontTables {
    std::vector<unsigned> ob, oe;
    std::vector<SumPass> passes;
    int64_t nmax = 0;
};

// the argument checks of both forms, and the tables
int sum_tables(const mce_summary_seg* segs, int32_t nseg, const double* q, int32_t nq, int64_t pass_elems, SumTables& T)
{
    int rc = sum_front_args("param summary", segs && q, nseg);
    if (rc != MCE_OK) return rc;
    if (nq < 1 || nq > MCE_SUMMARY_MAX_Q) return fail(MCE_ERR_INVALID, "param summary: %d targets (1 .. %d expected)", nq, MCE_SUMMARY_MAX_Q);
    for (int32_t t = 0; t < nq; ++t)
        if (!(q[t] > 0.0 && q[t] < 1.0)) return fail(MCE_ERR_INVALID, "param summary: target %d is %g (0 < q < 1 expected)", t, q[t]);
    if (pass_elems < 0 || pass_elems > kSumMaxRows) return fail(MCE_ERR_INVALID, "param summary: pass_elems=%lld", (long long)pass_elems);
    rc = sum_front_tables("param summary", segs, nseg, T, SumFrontNoCheck{}, [&](int32_t s, const mce_summary_seg& g) {
        if (g.n > 0) T.segs[(size_t)s].fs = g.fs;
        T.nmax = std::max(T.nmax, g.n);
        return mce_sum::sum_out_doubles(g.d, nq);
    });
    if (rc != MCE_OK) return rc;
    // the passes: runs in (system, column) order while they fit; a run longer than pass_elems is a pass of its own
    const int64_t pe = sum_pass_elems(pass_elems);
    SumPass cur;
    for (size_t r = 0; r < T.runs.size(); ++r) {
        const int64_t n = T.segs[(size_t)T.runs[r].seg].n;
        if (cur.nruns > 0 && cur.total + n > pe) {
            T.passes.push_back(cur);
            cur = SumPass{(int64_t)r, 0, 0, 0};
        }
        T.runs[r].begin = cur.total;
        T.runs[r].tile0 = cur.ntiles;
        T.ob.push_back((unsigned)cur.total);
        T.oe.push_back((unsigned)(cur.total + n));
        cur.nruns += 1;
        cur.total += n;
        cur.ntiles += (n + mce::kSumScanTile - 1) / mce::kSumScanTile;
    }
    if (cur.nruns > 0) T.passes.push_back(cur);
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
    MCE_HIP(hipMemcpyAsync(W.ob, T.ob.data(), T.ob.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.oe, T.oe.data(), T.oe.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(W.q, q, (size_t)nq * 8, hipMemcpyHostToDevice, st));
    if ((rc = sum_front_launch(W, T, nseg, true, st)) != MCE_OK) return rc;
    MCE_HIP(hipGetLastError());
    const dim3 tb(kPsumThreads);
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
    return seg_dev_end(out, W.res, (size_t)T.out_doubles, st);
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
