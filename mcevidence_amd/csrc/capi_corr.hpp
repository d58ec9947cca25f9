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

// the workspace of a chain of n rows in nparts parts, ndim columns, lags up to max_lag: the select workspace of the chain first
struct CorrWs {
    char* sel;
    size_t sel_bytes;
    mce::CorrPart* parts;
    long long* ends;
    double *mtiles, *mean, *ntau, *S, *rho;
    mce::CorrState* state;
    double* partial;
    size_t total;
    int64_t lag_rows, max_chunks, mean_chunks;
    CorrWs(int64_t n, int32_t nparts, int32_t ndim, int64_t max_lag, void* ws = nullptr)
    {
        lag_rows = max_lag + 1 + kCorrMaxLaunchLags;             // (a window may run past the cap; its lags are summed and not used)
        max_chunks = (int64_t)nparts * corr_chunks_per_part(nparts);
        mean_chunks = n / mce::kCorrMeanRows + nparts;
        sel_bytes = PrepWs(n, nparts).total;
        WsPlan P(ws);
        sel = P.take_bytes<char>(sel_bytes);
        parts = P.take<mce::CorrPart>((size_t)nparts);
        ends = P.take<long long>((size_t)nparts);
        mtiles = P.take<double>((size_t)mean_chunks * ndim * 3);
        mean = P.take<double>((size_t)nparts * ndim);
        ntau = P.take<double>((size_t)lag_rows);
        S = P.take<double>((size_t)lag_rows * ndim);
        rho = P.take<double>((size_t)lag_rows * ndim);
        state = P.take<mce::CorrState>((size_t)ndim);
        partial = P.take<double>((size_t)max_chunks * ndim * kCorrMaxLaunchLags);
        total = P.total;
    }
};

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
    return CorrWs(n, nparts, ndim, max_lag).total;
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
    const CorrWs L(n, nparts, ndim, max_lag, ws);
    if (ws_bytes < L.total) return fail(MCE_ERR_WORKSPACE, "chain corr: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    *rule = 0; status[0] = status[1] = 0; *units = 0; *cap = 0; *rho_rows = 0;
    for (int32_t j = 0; j < ndim; ++j) { length[j] = 0.0; cut[j] = 0; }

    // ---- units: the weights, their prefix sums and the rule, as for thinlen = 2 ----------------------------------------------------------
    const PrepWs PL(n, nparts, L.sel);
    double totals[5];
    rc = mce_chain_weights_dev(parts, nparts, ncols, iw, mce_corr::kCorrRuleThinlen, rule, totals, L.sel, L.sel_bytes, stream);
    if (rc != MCE_OK) return rc;
    if (*rule < 0) return MCE_OK;                                  // a decline: the caller words it
    const int integer = *rule == mce_prep::kRuleInteger ? 1 : 0;
    const PrepPart* d_prep = PL.parts;
    const long long* d_c = PL.c;
    const int np = (int)table.size();
    std::vector<long long> ends((size_t)np, 0);
    if (integer) {
        hipLaunchKernelGGL(corr_ends_kernel, dim3((np + kCorrThreads - 1) / kCorrThreads), dim3(kCorrThreads), 0, st, d_prep, np, d_c, L.ends);
        MCE_HIP(hipGetLastError());
        MCE_HIP(hipMemcpyAsync(ends.data(), L.ends, (size_t)np * 8, hipMemcpyDeviceToHost, st));
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
    std::vector<double> ntau((size_t)L.lag_rows, 0.0);
    for (int64_t t = 0; t < L.lag_rows; ++t) {
        int64_t cnt = 0;
        for (int p = 0; p < np; ++p) cnt += std::max<int64_t>(part_units[(size_t)p] - t, 0);
        ntau[(size_t)t] = (double)cnt;
    }
    MCE_HIP(hipMemcpyAsync(L.parts, cp.data(), cp.size() * sizeof(CorrPart), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(L.ntau, ntau.data(), ntau.size() * 8, hipMemcpyHostToDevice, st));
    int cl = 1;
    while (cl < ndim) cl <<= 1;
    hipLaunchKernelGGL(corr_mean_tile_kernel, dim3((unsigned)mchunks), dim3(kCorrThreads), 0, st, L.parts, np, ncols, (int)iw, (int)itheta, (int)ndim, cl, integer,
                       L.mtiles);
    hipLaunchKernelGGL(corr_mean_final_kernel, dim3((unsigned)(((int64_t)np * ndim + kCorrThreads - 1) / kCorrThreads)), dim3(kCorrThreads), 0, st, L.parts, np,
                       (int)ndim, L.mtiles, L.mean);
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
            hipLaunchKernelGGL(corr_lag_kernel, dim3((unsigned)nchunks, colgroups, (unsigned)nsub), dim3(kCorrThreads), 0, st, L.parts, np, d_c, integer, ncols,
                               (int)itheta, (int)ndim, L.mean, t, nlag, L.partial);
            hipLaunchKernelGGL(corr_reduce_kernel, dim3((unsigned)(((int64_t)ndim * nlag + kCorrThreads - 1) / kCorrThreads)), dim3(kCorrThreads), 0, st, L.partial,
                               nchunks, (int)ndim, nlag, t, L.S);
        }
        hipLaunchKernelGGL(corr_scan_kernel, dim3(1), dim3(kCorrThreads), 0, st, L.S, L.ntau, (int)ndim, tau0, tau1, min_corr, L.rho, L.state);
        MCE_HIP(hipGetLastError());
        MCE_HIP(hipMemcpyAsync(state.data(), L.state, state.size() * sizeof(CorrState), hipMemcpyDeviceToHost, st));
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
        MCE_HIP(hipMemcpyAsync(rho, L.rho, (size_t)*rho_rows * ndim * 8, hipMemcpyDeviceToHost, st));
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
