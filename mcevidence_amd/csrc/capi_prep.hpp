// capi_prep.hpp -- part of capi.hip (one translation unit): mce_chain_weights_dev / _select_count_dev / _select_fill_dev /
// _gather_dev / _reduce_dev: a chain that the reader left on the device is burned, concatenated, thinned, split and reduced there
// (chain_prep_kernels.hpp has the passes, chain_prep.hpp the rules).  Buffers and workspace are the caller's, everything runs on the
// caller's stream and on the caller's current device; the select workspace carries the weights, their prefix sums and the
// candidates from call to call, so the three select calls of one chain take the SAME workspace.  Argument checks come before any
// device call (MCE_ERR_INVALID without a GPU); compute without a device is MCE_ERR_NO_DEVICE.
#pragma once

#include "chain_prep.hpp"
#include "chain_prep_kernels.hpp"

namespace {

constexpr int32_t kPrepMaxParts = 65536;

template <class T> T* prep_at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

// (WsPlan, the planner of every workspace, and prep_align: ws_plan.hpp)
// the select workspace of a chain of n rows in nparts parts: the parts, the totals, the weights, their prefix sums, the candidates
// (the bin rule: up to n + 1 bins) and seven per-tile arrays
struct PrepWs {
    mce::PrepPart* parts;
    mce::PrepTotals* tot;
    double *w, *tile_frac;
    long long *c, *cand, *tile_sum, *tile_max, *tile_bad, *tile_base, *tile_cnt, *tile_out;
    size_t total;
    PrepWs(int64_t n, int32_t nparts, void* ws = nullptr)
    {
        const size_t ntl = (size_t)((n + 1 + mce::kPrepTile - 1) / mce::kPrepTile);
        WsPlan P(ws);
        parts = P.take<mce::PrepPart>((size_t)nparts);
        tot = P.take<mce::PrepTotals>(1);
        w = P.take<double>((size_t)n);
        c = P.take<long long>((size_t)n);
        cand = P.take<long long>((size_t)(n + 1));
        tile_sum = P.take<long long>(ntl);
        tile_max = P.take<long long>(ntl);
        tile_bad = P.take<long long>(ntl);
        tile_base = P.take<long long>(ntl);
        tile_frac = P.take<double>(ntl);
        tile_cnt = P.take<long long>(ntl);
        tile_out = P.take<long long>(ntl);
        total = P.total;
    }
};

// one entry of a part table (`who`: the caller's prefix): rows at a null pointer, negative rows, rows beyond 2^40
int prep_check_part(const char* who, long long p, const mce_chain_part& part)
{
    if (part.nrows < 0 || (part.nrows > 0 && !part.rows))
        return fail(MCE_ERR_INVALID, "%s: part %lld has %lld rows at a %s pointer", who, p, (long long)part.nrows, part.rows ? "valid" : "null");
    if (part.nrows > (int64_t)1 << 40) return fail(MCE_ERR_INVALID, "%s: part %lld has %lld rows", who, p, (long long)part.nrows);
    return MCE_OK;
}

// the table of non-empty parts and the total row count
int prep_parts(const mce_chain_part* parts, int32_t nparts, int64_t ncols, std::vector<mce::PrepPart>& table, int64_t& n)
{
    if (!parts || nparts < 1 || nparts > kPrepMaxParts) return fail(MCE_ERR_INVALID, "chain prep: %d parts (1 .. %d expected)", nparts, kPrepMaxParts);
    if (ncols < 1 || ncols > (1 << 20)) return fail(MCE_ERR_INVALID, "chain prep: ncols=%lld", (long long)ncols);
    n = 0;
    table.clear();
    for (int32_t p = 0; p < nparts; ++p) {
        const int rc = prep_check_part("chain prep", p, parts[p]);
        if (rc != MCE_OK) return rc;
        if (parts[p].nrows > 0) table.push_back(mce::PrepPart{parts[p].rows, n, parts[p].nrows});
        n += parts[p].nrows;
    }
    return MCE_OK;
}

int prep_need_device()
{
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) return fail(MCE_ERR_NO_DEVICE, "no HIP device visible");
    return MCE_OK;
}

int prep_select_args(int64_t n, int32_t nparts, int32_t rule, double thinlen, void* ws, size_t ws_bytes)
{
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (n < 1 || nparts < 1 || nparts > kPrepMaxParts) return fail(MCE_ERR_INVALID, "chain prep: n=%lld nparts=%d", (long long)n, nparts);
    if (rule != mce_prep::kRuleInteger && rule != mce_prep::kRuleBin) return fail(MCE_ERR_INVALID, "chain prep: rule %d selects nothing", rule);
    if (!(thinlen > 1.0)) return fail(MCE_ERR_INVALID, "chain prep: thinlen=%g", thinlen);
    const size_t need = PrepWs(n, nparts).total;
    if (ws_bytes < need) return fail(MCE_ERR_WORKSPACE, "chain prep: workspace of %zu bytes, %zu needed", ws_bytes, need);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_chain_select_workspace_bytes(int64_t n, int32_t nparts)
{
    if (n < 0 || nparts < 1 || nparts > kPrepMaxParts) return 0;
    return PrepWs(n, nparts).total;
}

size_t mce_chain_gather_workspace_bytes(int32_t nparts)
{
    if (nparts < 1 || nparts > kPrepMaxParts) return 0;
    return prep_align((size_t)nparts * sizeof(mce::PrepPart));
}

size_t mce_chain_reduce_workspace_bytes(int64_t n)
{
    if (n < 0) return 0;
    const size_t nt = (size_t)((n + mce::kPrepTile - 1) / mce::kPrepTile);
    return 3 * prep_align(std::max<size_t>(nt, 1) * 8) + prep_align(4 * sizeof(double));
}

int mce_chain_weights_dev(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, double thinlen, int32_t* rule, double* totals,
                          void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!rule || !totals || !ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<PrepPart> table;
    int64_t n = 0;
    int rc = prep_parts(parts, nparts, ncols, table, n);
    if (rc != MCE_OK) return rc;
    if (iw < 0 || iw >= ncols) return fail(MCE_ERR_INVALID, "chain prep: weight column %d of %lld", iw, (long long)ncols);
    if (n < 1) return fail(MCE_ERR_INVALID, "chain prep: no rows");
    const PrepWs W(n, nparts, ws);
    if (ws_bytes < W.total) return fail(MCE_ERR_WORKSPACE, "chain prep: workspace of %zu bytes, %zu needed", ws_bytes, W.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nt = (n + kPrepTile - 1) / kPrepTile;
    MCE_HIP(hipMemcpyAsync(W.parts, table.data(), table.size() * sizeof(PrepPart), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemsetAsync(W.tot, 0, sizeof(PrepTotals), st));
    hipLaunchKernelGGL(prep_weights_kernel, dim3(prep_grid(n, kPrepThreads)), dim3(kPrepThreads), 0, st, W.parts, (int)table.size(), n, ncols, (int)iw, W.w);
    hipLaunchKernelGGL(prep_tile_kernel, dim3(prep_grid(nt, 1)), dim3(kPrepThreads), 0, st, W.w, n, nt, W.tile_sum,
                       W.tile_max, W.tile_frac, W.tile_bad);
    hipLaunchKernelGGL(prep_scan_kernel, dim3(1), dim3(kPrepScanThreads), 0, st, W.tile_sum, nt,
                       W.tile_base, &W.tot->sum_int);
    hipLaunchKernelGGL(prep_totals_kernel, dim3(1), dim3(kPrepThreads), 0, st, W.tile_max, W.tile_frac,
                       W.tile_bad, nt, W.tot);
    hipLaunchKernelGGL(prep_cum_kernel, dim3(prep_grid(nt, 1)), dim3(kPrepThreads), 0, st, W.w, n, nt, W.tile_base,
                       W.c);
    MCE_HIP(hipGetLastError());
    PrepTotals tot;
    MCE_HIP(hipMemcpyAsync(&tot, W.tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    mce_prep::WeightTotals t;
    t.sum_int = tot.sum_int; t.max_int = tot.max_int; t.frac = tot.frac; t.bad = tot.bad;
    *rule = mce_prep::choose_rule(thinlen, t);
    totals[0] = (double)n; totals[1] = (double)tot.sum_int; totals[2] = (double)tot.max_int; totals[3] = tot.frac; totals[4] = (double)tot.bad;
    return MCE_OK;
}

int mce_chain_select_count_dev(int64_t n, int32_t nparts, int32_t rule, double thinlen, const double* d_edges, int64_t nedges, int64_t* n_out,
                               void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!n_out) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = prep_select_args(n, nparts, rule, thinlen, ws, ws_bytes);
    if (rc != MCE_OK) return rc;
    const PrepWs W(n, nparts, ws);
    if (rule == mce_prep::kRuleBin && (!d_edges || nedges < 1 || nedges > n + 1))
        return fail(MCE_ERR_INVALID, "chain prep: the bin rule needs 1 .. n + 1 edges on the device (got %lld)", (long long)nedges);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PrepTotals* d_tot = W.tot;
    PrepTotals tot;
    MCE_HIP(hipMemcpyAsync(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    long long* cand = W.cand;
    int64_t len = n;
    if (rule == mce_prep::kRuleInteger) {
        const long long factor = (long long)thinlen;
        if (factor < tot.max_int) {          // second branch: the count is known, nothing to flag
            *n_out = tot.sum_int / factor;
            return MCE_OK;
        }
        hipLaunchKernelGGL(prep_flag_kernel, dim3(prep_grid(n, kPrepThreads)), dim3(kPrepThreads), 0, st, W.c, n, factor, cand);
    } else {
        len = nedges;
        hipLaunchKernelGGL(prep_bin_kernel, dim3(prep_grid(nedges, kPrepThreads / 64)), dim3(kPrepThreads), 0, st, W.w, n, d_edges,
                           nedges, cand);
    }
    const int64_t nt = (len + kPrepTile - 1) / kPrepTile;
    hipLaunchKernelGGL(prep_count_kernel, dim3(prep_grid(nt, 1)), dim3(kPrepThreads), 0, st, cand, len, nt, W.tile_cnt);
    hipLaunchKernelGGL(prep_scan_kernel, dim3(1), dim3(kPrepScanThreads), 0, st, W.tile_cnt, nt,
                       W.tile_out, &d_tot->n_out);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(&tot, d_tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    *n_out = tot.n_out;
    return MCE_OK;
}

int mce_chain_select_fill_dev(int64_t n, int32_t nparts, int32_t rule, double thinlen, int64_t nedges, int64_t n_out, int64_t* d_src, double* d_new_w,
                              void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!d_src || !d_new_w) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = prep_select_args(n, nparts, rule, thinlen, ws, ws_bytes);
    if (rc != MCE_OK) return rc;
    const PrepWs W(n, nparts, ws);
    if (n_out < 1) return fail(MCE_ERR_INVALID, "chain prep: n_out=%lld", (long long)n_out);
    if (rule == mce_prep::kRuleBin && (nedges < 1 || nedges > n + 1)) return fail(MCE_ERR_INVALID, "chain prep: %lld edges", (long long)nedges);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PrepTotals tot;
    MCE_HIP(hipMemcpyAsync(&tot, W.tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    const long long factor = (long long)thinlen;
    const double* d_w = W.w;
    if (rule == mce_prep::kRuleInteger && factor < tot.max_int) {
        if (n_out != tot.sum_int / factor) return fail(MCE_ERR_INVALID, "chain prep: n_out=%lld, the count call said %lld", (long long)n_out, tot.sum_int / factor);
        hipLaunchKernelGGL(prep_search_kernel, dim3(prep_grid(n_out, kPrepThreads)), dim3(kPrepThreads), 0, st, W.c, n, factor, n_out,
                           d_w, reinterpret_cast<long long*>(d_src), d_new_w);
    } else {
        if (n_out != tot.n_out) return fail(MCE_ERR_INVALID, "chain prep: n_out=%lld, the count call said %lld", (long long)n_out, tot.n_out);
        const int64_t len = rule == mce_prep::kRuleInteger ? n : nedges;
        const int64_t nt = (len + kPrepTile - 1) / kPrepTile;
        hipLaunchKernelGGL(prep_fill_kernel, dim3(prep_grid(nt, 1)), dim3(kPrepThreads), 0, st, W.cand, len, nt,
                           W.tile_out, d_w, rule == mce_prep::kRuleInteger ? 1 : 0, n_out, reinterpret_cast<long long*>(d_src),
                           d_new_w);
    }
    MCE_HIP(hipGetLastError());
    return MCE_OK;
}

int mce_chain_gather_dev(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, int32_t ilike, int32_t itheta, const int64_t* d_src,
                         const double* d_new_w, int64_t n_thin, const int64_t* d_rows, int64_t n_out, double* d_params, double* d_w, double* d_like,
                         double* d_full, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!ws || (!d_params && !d_w && !d_like && !d_full)) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<PrepPart> table;
    int64_t n = 0;
    int rc = prep_parts(parts, nparts, ncols, table, n);
    if (rc != MCE_OK) return rc;
    if (iw < 0 || ilike < 0 || itheta < 0 || ncols <= std::max(iw, std::max(ilike, itheta)))
        return fail(MCE_ERR_INVALID, "chain prep: columns iw=%d ilike=%d itheta=%d of %lld", iw, ilike, itheta, (long long)ncols);
    if (n < 1 || n_out < 1 || n_thin < 1) return fail(MCE_ERR_INVALID, "chain prep: n=%lld n_thin=%lld n_out=%lld", (long long)n, (long long)n_thin, (long long)n_out);
    if (!d_src && (n_thin != n || d_new_w)) return fail(MCE_ERR_INVALID, "chain prep: without a row list the thinned chain is the chain itself");
    if (!d_rows && n_out != n_thin) return fail(MCE_ERR_INVALID, "chain prep: without an index list n_out = n_thin");
    if (n_out > INT64_MAX / ncols) return fail(MCE_ERR_INVALID, "chain prep: n_out=%lld", (long long)n_out);
    const size_t need = prep_align((size_t)nparts * sizeof(PrepPart));
    if (ws_bytes < need) return fail(MCE_ERR_WORKSPACE, "chain prep: workspace of %zu bytes, %zu needed", ws_bytes, need);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PrepPart* d_parts = static_cast<PrepPart*>(ws);
    MCE_HIP(hipMemcpyAsync(d_parts, table.data(), table.size() * sizeof(PrepPart), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(prep_gather_kernel, dim3(prep_grid(n_out * ncols, kPrepThreads)), dim3(kPrepThreads), 0, st, d_parts, (int)table.size(), n, ncols, (int)iw,
                       (int)ilike, (int)itheta, reinterpret_cast<const long long*>(d_src), d_new_w, n_thin, reinterpret_cast<const long long*>(d_rows), n_out,
                       d_params, d_w, d_like, d_full);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipStreamSynchronize(st));          // (the table came from this call's own memory; the feed wants a synchronised stream anyway)
    return MCE_OK;
}

int mce_chain_reduce_dev(const double* d_like, const double* d_w, int64_t n, int32_t pos_lnp, double* d_fs, double* out, void* ws, size_t ws_bytes,
                         void* stream)
{
    using namespace mce;
    if (!d_like || !d_w || !d_fs || !out || !ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (n < 1) return fail(MCE_ERR_INVALID, "chain prep: n=%lld", (long long)n);
    const size_t need = mce_chain_reduce_workspace_bytes(n);
    if (ws_bytes < need) return fail(MCE_ERR_WORKSPACE, "chain prep: workspace of %zu bytes, %zu needed", ws_bytes, need);
    int rc = prep_need_device();
    if (rc != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nt = (n + kPrepTile - 1) / kPrepTile;
    const size_t seg = prep_align((size_t)nt * 8);
    double* t_max = prep_at<double>(ws, 0);
    double* t_sum = prep_at<double>(ws, seg);
    long long* t_bad = prep_at<long long>(ws, 2 * seg);
    double* red = prep_at<double>(ws, 3 * seg);
    hipLaunchKernelGGL(prep_like_tile_kernel, dim3(prep_grid(nt, 1)), dim3(kPrepThreads), 0, st, d_like, d_w, n, nt, (int)(pos_lnp != 0), t_max, t_sum, t_bad);
    hipLaunchKernelGGL(prep_like_final_kernel, dim3(1), dim3(kPrepThreads), 0, st, t_max, t_sum, t_bad, nt, red);
    hipLaunchKernelGGL(prep_fs_kernel, dim3(prep_grid(n, kPrepThreads)), dim3(kPrepThreads), 0, st, d_like, n, (int)(pos_lnp != 0), red, d_fs);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, red, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    return MCE_OK;
}

}  // extern "C"
