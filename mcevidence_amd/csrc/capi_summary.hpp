// capi_summary.hpp -- part of capi.hip (one translation unit): mce_param_summary_out_doubles / mce_param_summary_workspace_bytes /
// mce_param_summary_dev / mce_param_summary_f64: the posterior summary (weighted means, variances, extremes, weighted quantiles, best
// fit) of the parameter columns of MANY systems (the ready roots of a farm wave) that are on the device, in one call
// (param_summary_kernels.hpp has the launches, param_summary.hpp the rule).  Everything is enqueued on the caller's stream; the host
// waits once, for one block of results.  Argument checks come before any device call.  The runs (system, column) are sorted in PASSES
// of at most pass_elems elements, so the number of launches depends on the number of passes, not on the number of systems.
#pragma once

#include <rocprim/device/device_segmented_radix_sort.hpp>

#include "param_summary.hpp"
#include "param_summary_kernels.hpp"

namespace {

constexpr int32_t kSumMaxSegs = 1 << 16;
constexpr int64_t kSumMaxRows = 0x7fffffffLL;                   // (rocPRIM's segmented sort counts a pass in 32 bits)

struct SumLayout {
    size_t off_segs = 0, off_tile0 = 0, off_head = 0, off_cols = 0, off_part = 0, off_sys = 0, off_col = 0, off_quant = 0, off_q = 0, off_runs = 0, off_ob = 0,
           off_oe = 0, off_tot = 0, off_res = 0, off_keys[2] = {0, 0}, off_wts[2] = {0, 0}, off_tmp = 0, tmp_bytes = 0, total = 0;
    int64_t max_tiles = 0, cap = 0, max_runs = 0, max_scan = 0;
};

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

SumLayout sum_layout(int64_t nrows_total, int64_t nrows_max, int32_t nseg, int32_t dmax, int32_t nq, int64_t pass_elems)
{
    SumLayout L;
    L.max_tiles = nrows_total / mce::kSumTileRows + nseg;
    // a pass holds at most pass_elems elements, or one run; never more than there are elements at all
    L.cap = std::max<int64_t>(std::max(std::min(sum_pass_elems(pass_elems), nrows_total * dmax), nrows_max), 1);
    L.max_runs = (int64_t)nseg * dmax;
    L.max_scan = L.cap / mce::kSumScanTile + L.max_runs + 1;
    const size_t S = (size_t)nseg, T = (size_t)L.max_tiles, R = (size_t)L.max_runs, D = (size_t)dmax;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += prep_align(bytes); return at; };
    L.off_segs = take(S * sizeof(mce::SumSeg));
    L.off_tile0 = take(S * sizeof(int64_t));
    L.off_head = take(T * mce::kSumTileHead * 8);
    L.off_cols = take(T * mce::kSumTileCol * D * 8);
    L.off_part = take(T * D * 8);
    L.off_sys = take(S * mce::kSumSys * 8);
    L.off_col = take(R * mce::kSumCol * 8);
    L.off_quant = take(R * (size_t)nq * 8);
    L.off_q = take((size_t)MCE_SUMMARY_MAX_Q * 8);
    L.off_runs = take(R * sizeof(mce::SumRun));
    L.off_ob = take(R * sizeof(unsigned));
    L.off_oe = take(R * sizeof(unsigned));
    L.off_tot = take((size_t)L.max_scan * 8);
    L.off_res = take(S * (size_t)mce_sum::sum_out_doubles(dmax, nq) * 8);
    for (int k = 0; k < 2; ++k) L.off_keys[k] = take((size_t)L.cap * 8);
    for (int k = 0; k < 2; ++k) L.off_wts[k] = take((size_t)L.cap * 8);
    L.tmp_bytes = prep_align(sum_sort_tmp_bytes(L.cap, L.max_runs));
    L.off_tmp = take(L.tmp_bytes);
    L.total = off;
    return L;
}

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
    std::vector<int64_t> tile0;
    std::vector<mce::SumRun> runs;
    std::vector<unsigned> ob, oe;
    std::vector<SumPass> passes;
    int64_t nrows = 0, nmax = 0, ntiles = 0, out_doubles = 0;
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
    T.tile0.assign((size_t)nseg, 0);
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
        T.tile0[(size_t)s] = T.ntiles;
        T.ntiles += (g.n + mce::kSumTileRows - 1) / mce::kSumTileRows;
        T.nrows += g.n;
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
    if (T.ntiles > 0x7fffffffLL) return fail(MCE_ERR_INVALID, "param summary: %lld rows in one call", (long long)T.nrows);
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
    return sum_layout(nrows_total, nrows_max, nseg, dmax, nq, pass_elems).total;
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
    const SumLayout L = sum_layout(T.nrows, T.nmax, nseg, T.dmax, nq, pass_elems);
    if (ws_bytes < L.total) return fail(MCE_ERR_WORKSPACE, "param summary: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int dmax = T.dmax;
    const int64_t R = (int64_t)T.runs.size();

    SumSeg* d_segs = prep_at<SumSeg>(ws, L.off_segs);
    int64_t* d_tile0 = prep_at<int64_t>(ws, L.off_tile0);
    double* d_head = prep_at<double>(ws, L.off_head);
    double* d_cols = prep_at<double>(ws, L.off_cols);
    double* d_part = prep_at<double>(ws, L.off_part);
    double* d_sys = prep_at<double>(ws, L.off_sys);
    double* d_col = prep_at<double>(ws, L.off_col);
    double* d_quant = prep_at<double>(ws, L.off_quant);
    double* d_q = prep_at<double>(ws, L.off_q);
    SumRun* d_runs = prep_at<SumRun>(ws, L.off_runs);
    unsigned* d_ob = prep_at<unsigned>(ws, L.off_ob);
    unsigned* d_oe = prep_at<unsigned>(ws, L.off_oe);
    double* d_tot = prep_at<double>(ws, L.off_tot);
    double* d_res = prep_at<double>(ws, L.off_res);

    MCE_HIP(hipMemcpyAsync(d_segs, T.segs.data(), T.segs.size() * sizeof(SumSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_tile0, T.tile0.data(), T.tile0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_runs, T.runs.data(), T.runs.size() * sizeof(SumRun), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_ob, T.ob.data(), T.ob.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_oe, T.oe.data(), T.oe.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_q, q, (size_t)nq * 8, hipMemcpyHostToDevice, st));
    const dim3 tb(kPsumThreads);
    const unsigned ntiles = (unsigned)T.ntiles;
    if (ntiles > 0) hipLaunchKernelGGL(sum_tile_kernel, dim3(ntiles), tb, 0, st, d_segs, d_tile0, (int)nseg, dmax, d_head, d_cols);
    hipLaunchKernelGGL(sum_sys_kernel, dim3((unsigned)nseg), tb, 0, st, d_segs, d_tile0, d_head, d_sys);
    hipLaunchKernelGGL(sum_col_kernel, dim3((unsigned)R), tb, 0, st, d_segs, d_tile0, d_runs, dmax, d_cols, d_sys, d_col);
    if (ntiles > 0) hipLaunchKernelGGL(sum_var_tile_kernel, dim3(ntiles), tb, 0, st, d_segs, d_tile0, (int)nseg, dmax, d_col, d_part);
    hipLaunchKernelGGL(sum_var_col_kernel, dim3((unsigned)R), tb, 0, st, d_segs, d_tile0, d_runs, dmax, d_part, d_sys, d_col);
    MCE_HIP(hipGetLastError());
    for (const SumPass& P : T.passes) {
        if (P.total > L.cap || P.ntiles > L.max_scan) return fail(MCE_ERR_WORKSPACE, "param summary: a pass of %lld elements, %lld planned", (long long)P.total, (long long)L.cap);
        rocprim::double_buffer<unsigned long long> keys(prep_at<unsigned long long>(ws, L.off_keys[0]), prep_at<unsigned long long>(ws, L.off_keys[1]));
        rocprim::double_buffer<double> wts(prep_at<double>(ws, L.off_wts[0]), prep_at<double>(ws, L.off_wts[1]));
        const SumRun* p_runs = d_runs + P.run0;
        if (P.total > 0) {
            hipLaunchKernelGGL(sum_keys_kernel, dim3((unsigned)((P.total + kPsumThreads - 1) / kPsumThreads)), tb, 0, st, d_segs, p_runs, (int)P.nruns, P.total,
                               keys.current(), wts.current());
            size_t need = 0;
            MCE_HIP(rocprim::segmented_radix_sort_pairs(nullptr, need, keys, wts, (unsigned)P.total, (unsigned)P.nruns, d_ob + P.run0, d_oe + P.run0, 0u, 64u, st));
            if (need > L.tmp_bytes) return fail(MCE_ERR_WORKSPACE, "param summary: the sort asks for %zu bytes, %zu planned", need, L.tmp_bytes);
            need = L.tmp_bytes;
            MCE_HIP(rocprim::segmented_radix_sort_pairs(prep_at<void>(ws, L.off_tmp), need, keys, wts, (unsigned)P.total, (unsigned)P.nruns, d_ob + P.run0,
                                                        d_oe + P.run0, 0u, 64u, st));
            hipLaunchKernelGGL(sum_scan_tile_kernel, dim3((unsigned)P.ntiles), tb, 0, st, d_segs, p_runs, (int)P.nruns, wts.current(), d_tot);
        }
        hipLaunchKernelGGL(sum_search_kernel, dim3((unsigned)P.nruns), dim3(64), 0, st, d_segs, p_runs, P.run0, d_q, (int)nq, d_sys, keys.current(), wts.current(),
                           d_tot, d_quant);
        MCE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(sum_result_kernel, dim3((unsigned)nseg), tb, 0, st, d_segs, d_sys, d_col, d_quant, (int)nq, d_res);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, d_res, (size_t)T.out_doubles * 8, hipMemcpyDeviceToHost, st));
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
    size_t elems = 1;
    for (int32_t s = 0; s < nseg; ++s) elems += (size_t)segs[s].n * ((size_t)segs[s].d + 2);
    DevBuf data, ws;
    MCE_HIP(data.alloc(elems * sizeof(double)));
    std::vector<mce_summary_seg> dsegs((size_t)nseg);
    double* at = data.as<double>();
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_summary_seg& g = segs[s];
        const size_t n = (size_t)g.n, d = (size_t)g.d;
        mce_summary_seg o = g;
        o.x = nullptr; o.w = nullptr; o.fs = nullptr; o.ld = g.d;
        if (n > 0) {
            // the d measured columns, packed: ld = d on the device
            MCE_HIP(hipMemcpy2D(at, d * 8, g.x, (size_t)g.ld * 8, d * 8, n, hipMemcpyHostToDevice));
            o.x = at; at += n * d;
            MCE_HIP(hipMemcpy(at, g.w, n * 8, hipMemcpyHostToDevice));
            o.w = at; at += n;
            if (g.fs) {
                MCE_HIP(hipMemcpy(at, g.fs, n * 8, hipMemcpyHostToDevice));
                o.fs = at; at += n;
            }
        }
        dsegs[(size_t)s] = o;
    }
    const size_t wsb = mce_param_summary_workspace_bytes(T.nrows, T.nmax, nseg, T.dmax, nq, pass_elems);
    MCE_HIP(ws.alloc(wsb));
    return mce_param_summary_dev(dsegs.data(), nseg, q, nq, pass_elems, out, ws.p, wsb, nullptr);
}

}  // extern "C"
