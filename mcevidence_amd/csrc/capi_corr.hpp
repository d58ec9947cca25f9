// capi_corr.hpp -- part of capi.hip (one translation unit): mce_chain_corr_workspace_bytes / mce_chain_corr_dev / mce_chain_corr_f64: the
// pooled, per-parameter autocorrelation length of burned chains that are on the device (chain_corr_kernels.hpp has the passes,
// chain_corr.hpp the rule).  The weights, their prefix sums and the rule come from mce_chain_weights_dev (thinlen 2), which takes the
// head of the workspace.  Lags are summed in windows that double -- 128, 256, 512, .. lags, capped by the lags left --, a window as
// launches of at most 256 lags on the stream (the partial sums of one launch are reduced before the next reuses their buffer); after
// each WINDOW the host reads one small block per column and stops once every column has its cut: at most log2(cap / 128) + 1 waits.  Argument checks come before any device call.
#pragma once

#include "chain_corr.hpp"
#include "chain_corr_kernels.hpp"

namespace {

constexpr int64_t kCorrMaxLagArg = 65536;
constexpr int kCorrMaxLaunchLags = 2 * mce::kCorrWin;            // lags per launch (the partial sums of one launch are kept)
constexpr int64_t kCorrChunksPerPart = 64;                       // up to 64 parts; beyond, 4096 chunks are shared out
constexpr int64_t kCorrChunkBudget = 4096;

int64_t corr_chunks_per_part(int32_t nparts) { return nparts <= 64 ? kCorrChunksPerPart : std::max<int64_t>(1, kCorrChunkBudget / nparts); }

struct CorrLayout {
    size_t off_sel = 0, off_parts = 0, off_ends = 0, off_mtiles = 0, off_mean = 0, off_ntau = 0, off_S = 0, off_rho = 0, off_state = 0, off_partial = 0, total = 0;
    int64_t lag_rows = 0, max_chunks = 0, mean_chunks = 0;
};

CorrLayout corr_layout(int64_t n, int32_t nparts, int32_t ndim, int64_t max_lag)
{
    CorrLayout L;
    L.lag_rows = max_lag + 1 + kCorrMaxLaunchLags;               // (a window may run past the cap; its lags are summed and not used)
    L.max_chunks = (int64_t)nparts * corr_chunks_per_part(nparts);
    L.mean_chunks = n / mce::kCorrMeanRows + nparts;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += prep_align(bytes); return at; };
    L.off_sel = take(prep_layout(n, nparts).total);
    L.off_parts = take((size_t)nparts * sizeof(mce::CorrPart));
    L.off_ends = take((size_t)nparts * 8);
    L.off_mtiles = take((size_t)L.mean_chunks * ndim * 3 * 8);
    L.off_mean = take((size_t)nparts * ndim * 8);
    L.off_ntau = take((size_t)L.lag_rows * 8);
    L.off_S = take((size_t)L.lag_rows * ndim * 8);
    L.off_rho = take((size_t)L.lag_rows * ndim * 8);
    L.off_state = take((size_t)ndim * sizeof(mce::CorrState));
    L.off_partial = take((size_t)L.max_chunks * ndim * kCorrMaxLaunchLags * 8);
    L.total = off;
    return L;
}

int corr_check_scalars(int64_t ncols, int32_t iw, int32_t itheta, int32_t ndim, double min_corr, int64_t max_lag)
{
    if (ncols < 1 || ncols > (1 << 20)) return fail(MCE_ERR_INVALID, "chain corr: ncols=%lld", (long long)ncols);
    if (iw < 0 || iw >= ncols || itheta < 0 || itheta >= ncols)
        return fail(MCE_ERR_INVALID, "chain corr: columns iw=%d itheta=%d of %lld", iw, itheta, (long long)ncols);
    if (ndim < 1 || ndim > mce::kCorrMaxDim || ndim > ncols - itheta)
        return fail(MCE_ERR_INVALID, "chain corr: ndim=%d (1 .. %d, and at most the %lld parameter columns)", ndim, mce::kCorrMaxDim, (long long)(ncols - itheta));
    if (!(min_corr >= 0.0 && min_corr < 1.0)) return fail(MCE_ERR_INVALID, "chain corr: min_corr=%g (0 <= min_corr < 1 expected)", min_corr);
    if (max_lag < 1 || max_lag > kCorrMaxLagArg) return fail(MCE_ERR_INVALID, "chain corr: max_lag=%lld (1 .. %lld expected)", (long long)max_lag, (long long)kCorrMaxLagArg);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_chain_corr_workspace_bytes(int64_t n, int32_t nparts, int32_t ndim, int64_t max_lag)
{
    if (n < 0 || nparts < 1 || nparts > kPrepMaxParts || ndim < 1 || ndim > mce::kCorrMaxDim || max_lag < 1 || max_lag > kCorrMaxLagArg) return 0;
    return corr_layout(n, nparts, ndim, max_lag).total;
}

int mce_chain_corr_dev(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, int32_t itheta, int32_t ndim, double min_corr,
                       int64_t max_lag, int32_t* rule, int32_t* status, int64_t* units, int64_t* cap, double* length, int64_t* cut, double* rho,
                       int64_t* rho_rows, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!rule || !status || !units || !cap || !length || !cut || !rho_rows || !ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<PrepPart> table;
    int64_t n = 0;
    int rc = prep_parts(parts, nparts, ncols, table, n);
    if (rc != MCE_OK) return rc;
    if ((rc = corr_check_scalars(ncols, iw, itheta, ndim, min_corr, max_lag)) != MCE_OK) return rc;
    if (n < 1) return fail(MCE_ERR_INVALID, "chain corr: no rows");
    const CorrLayout L = corr_layout(n, nparts, ndim, max_lag);
    if (ws_bytes < L.total) return fail(MCE_ERR_WORKSPACE, "chain corr: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    *rule = 0; status[0] = status[1] = 0; *units = 0; *cap = 0; *rho_rows = 0;
    for (int32_t j = 0; j < ndim; ++j) { length[j] = 0.0; cut[j] = 0; }

    // ---- units: the weights, their prefix sums and the rule, as for thinlen = 2 ----------------------------------------------------------
    char* sel = prep_at<char>(ws, L.off_sel);
    const PrepLayout PL = prep_layout(n, nparts);
    double totals[5];
    rc = mce_chain_weights_dev(parts, nparts, ncols, iw, mce_corr::kCorrRuleThinlen, rule, totals, sel, PL.total, stream);
    if (rc != MCE_OK) return rc;
    if (*rule < 0) return MCE_OK;                                  // a decline: the caller words it
    const int integer = *rule == mce_prep::kRuleInteger ? 1 : 0;
    const PrepPart* d_prep = reinterpret_cast<const PrepPart*>(sel + PL.off_parts);
    const long long* d_c = reinterpret_cast<const long long*>(sel + PL.off_c);
    const int np = (int)table.size();
    std::vector<long long> ends((size_t)np, 0);
    if (integer) {
        long long* d_ends = prep_at<long long>(ws, L.off_ends);
        hipLaunchKernelGGL(corr_ends_kernel, dim3((np + kCorrThreads - 1) / kCorrThreads), dim3(kCorrThreads), 0, st, d_prep, np, d_c, d_ends);
        MCE_HIP(hipGetLastError());
        MCE_HIP(hipMemcpyAsync(ends.data(), d_ends, (size_t)np * 8, hipMemcpyDeviceToHost, st));
        MCE_HIP(hipStreamSynchronize(st));
    }
    const int64_t cpp = corr_chunks_per_part(nparts);
    std::vector<CorrPart> cp((size_t)np);
    std::vector<int64_t> part_units((size_t)np);
    int64_t total_units = 0, max_units = 0, nchunks = 0, mchunks = 0;
    for (int p = 0; p < np; ++p) {
        CorrPart& q = cp[(size_t)p];
        q.rows = table[(size_t)p].rows;
        q.first = table[(size_t)p].first;
        q.nrows = table[(size_t)p].nrows;
        q.c_base = integer && p > 0 ? ends[(size_t)p - 1] : 0;
        q.units = integer ? ends[(size_t)p] - q.c_base : q.nrows;
        const int64_t ntiles = (q.units + kCorrTile - 1) / kCorrTile;
        q.tiles_per_chunk = (int32_t)std::max<int64_t>(1, (ntiles + cpp - 1) / cpp);
        q.pad = 0;
        q.chunk0 = nchunks;
        q.mchunk0 = mchunks;
        nchunks += (ntiles + q.tiles_per_chunk - 1) / q.tiles_per_chunk;
        mchunks += (q.nrows + kCorrMeanRows - 1) / kCorrMeanRows;
        part_units[(size_t)p] = q.units;
        total_units += q.units;
        max_units = std::max(max_units, q.units);
    }
    if (nchunks > L.max_chunks || mchunks > L.mean_chunks) return fail(MCE_ERR_WORKSPACE, "chain corr: %lld chunks of %lld", (long long)nchunks, (long long)L.max_chunks);
    *units = total_units;
    *cap = mce_corr::corr_cap(max_lag, max_units);
    if (*cap < 1) {                                                // (no lag to look at: no cut, at the first column)
        status[0] = mce_corr::kCorrNoCut;
        status[1] = 0;
        return MCE_OK;
    }

    // ---- (a) the centring values -----------------------------------------------------------------------------------------------------------
    CorrPart* d_parts = prep_at<CorrPart>(ws, L.off_parts);
    double* d_mtiles = prep_at<double>(ws, L.off_mtiles);
    double* d_mean = prep_at<double>(ws, L.off_mean);
    double* d_ntau = prep_at<double>(ws, L.off_ntau);
    double* d_S = prep_at<double>(ws, L.off_S);
    double* d_rho = prep_at<double>(ws, L.off_rho);
    CorrState* d_state = prep_at<CorrState>(ws, L.off_state);
    double* d_partial = prep_at<double>(ws, L.off_partial);
    std::vector<double> ntau((size_t)L.lag_rows, 0.0);
    for (int64_t t = 0; t < L.lag_rows; ++t) {
        int64_t cnt = 0;
        for (int p = 0; p < np; ++p) cnt += std::max<int64_t>(part_units[(size_t)p] - t, 0);
        ntau[(size_t)t] = (double)cnt;
    }
    MCE_HIP(hipMemcpyAsync(d_parts, cp.data(), cp.size() * sizeof(CorrPart), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_ntau, ntau.data(), ntau.size() * 8, hipMemcpyHostToDevice, st));
    int cl = 1;
    while (cl < ndim) cl <<= 1;
    hipLaunchKernelGGL(corr_mean_tile_kernel, dim3((unsigned)mchunks), dim3(kCorrThreads), 0, st, d_parts, np, ncols, (int)iw, (int)itheta, (int)ndim, cl, integer,
                       d_mtiles);
    hipLaunchKernelGGL(corr_mean_final_kernel, dim3((unsigned)(((int64_t)np * ndim + kCorrThreads - 1) / kCorrThreads)), dim3(kCorrThreads), 0, st, d_parts, np,
                       (int)ndim, d_mtiles, d_mean);
    MCE_HIP(hipGetLastError());

    // ---- (b), (c): windows of lags until every column has its cut --------------------------------------------------------------------------
    std::vector<CorrState> state((size_t)ndim);
    std::vector<double> s0((size_t)ndim);
    std::vector<int64_t> cuts((size_t)ndim, 0);
    int64_t tau0 = 0, column = -1;
    int code = mce_corr::kCorrOk;
    const unsigned colgroups = (unsigned)((ndim + kCorrCols - 1) / kCorrCols);
    for (int window = 0; tau0 <= *cap; ++window) {
        const int64_t wlags = (int64_t)kCorrWin << std::min(window, 20);
        const int64_t tau1 = std::min<int64_t>(tau0 + wlags - 1, *cap);
        for (int64_t t = tau0; t <= tau1; t += kCorrMaxLaunchLags) {          // (the last launch may run up to 255 lags past the cap: summed, not used)
            const int nsub = (int)std::min<int64_t>(kCorrMaxLaunchLags / kCorrWin, (tau1 + 1 - t + kCorrWin - 1) / kCorrWin);
            const int nlag = nsub * kCorrWin;
            hipLaunchKernelGGL(corr_lag_kernel, dim3((unsigned)nchunks, colgroups, (unsigned)nsub), dim3(kCorrThreads), 0, st, d_parts, np, d_c, integer, ncols,
                               (int)itheta, (int)ndim, d_mean, t, nlag, d_partial);
            hipLaunchKernelGGL(corr_reduce_kernel, dim3((unsigned)(((int64_t)ndim * nlag + kCorrThreads - 1) / kCorrThreads)), dim3(kCorrThreads), 0, st, d_partial,
                               nchunks, (int)ndim, nlag, t, d_S);
        }
        hipLaunchKernelGGL(corr_scan_kernel, dim3(1), dim3(kCorrThreads), 0, st, d_S, d_ntau, (int)ndim, tau0, tau1, min_corr, d_rho, d_state);
        MCE_HIP(hipGetLastError());
        MCE_HIP(hipMemcpyAsync(state.data(), d_state, state.size() * sizeof(CorrState), hipMemcpyDeviceToHost, st));
        MCE_HIP(hipStreamSynchronize(st));
        *rho_rows = tau1 + 1;
        for (int32_t j = 0; j < ndim; ++j) { s0[(size_t)j] = state[(size_t)j].s0; cuts[(size_t)j] = state[(size_t)j].cut; }
        code = mce_corr::corr_status(s0.data(), cuts.data(), ndim, &column);
        if (code != mce_corr::kCorrNoCut) break;                   // every cut found, or a column that cannot be measured
        tau0 = tau1 + 1;
    }
    status[0] = code;
    status[1] = (int32_t)(code == mce_corr::kCorrOk ? 0 : column);
    for (int32_t j = 0; j < ndim; ++j) {
        mce_corr::CorrColumn col;
        col.cut = state[(size_t)j].cut;
        col.sum = state[(size_t)j].sum;
        cut[j] = col.cut;
        length[j] = mce_corr::corr_length(col);
    }
    if (rho) {
        MCE_HIP(hipMemcpyAsync(rho, d_rho, (size_t)*rho_rows * ndim * 8, hipMemcpyDeviceToHost, st));
        MCE_HIP(hipStreamSynchronize(st));
    }
    return MCE_OK;
}

int mce_chain_corr_f64(const mce_chain_part* parts, int32_t nparts, int64_t ncols, int32_t iw, int32_t itheta, int32_t ndim, double min_corr,
                       int64_t max_lag, int32_t* rule, int32_t* status, int64_t* units, int64_t* cap, double* length, int64_t* cut, double* rho,
                       int64_t* rho_rows, int32_t device)
{
    if (!rule || !status || !units || !cap || !length || !cut || !rho_rows) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<mce::PrepPart> table;
    int64_t n = 0;
    int rc = prep_parts(parts, nparts, ncols, table, n);
    if (rc != MCE_OK) return rc;
    if ((rc = corr_check_scalars(ncols, iw, itheta, ndim, min_corr, max_lag)) != MCE_OK) return rc;
    if (n < 1) return fail(MCE_ERR_INVALID, "chain corr: no rows");
    if ((rc = select_device(device)) != MCE_OK) return rc;
    DevBuf rows, ws;
    MCE_HIP(rows.alloc((size_t)n * ncols * sizeof(double)));
    std::vector<mce_chain_part> dparts((size_t)nparts);
    int64_t at = 0;
    for (int32_t p = 0; p < nparts; ++p) {
        dparts[(size_t)p].rows = parts[p].nrows > 0 ? rows.as<double>() + at * ncols : nullptr;
        dparts[(size_t)p].nrows = parts[p].nrows;
        if (parts[p].nrows > 0)
            MCE_HIP(hipMemcpy(rows.as<double>() + at * ncols, parts[p].rows, (size_t)parts[p].nrows * ncols * sizeof(double), hipMemcpyHostToDevice));
        at += parts[p].nrows;
    }
    const size_t wsb = mce_chain_corr_workspace_bytes(n, nparts, ndim, max_lag);
    MCE_HIP(ws.alloc(wsb));
    return mce_chain_corr_dev(dparts.data(), nparts, ncols, iw, itheta, ndim, min_corr, max_lag, rule, status, units, cap, length, cut, rho, rho_rows, ws.p, wsb,
                              nullptr);
}

}  // extern "C"
