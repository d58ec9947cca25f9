// capi_moments.hpp -- part of capi.hip (one translation unit): mce_like_moments_workspace_bytes / mce_like_moments_dev /
// mce_like_moments_f64: the weighted moments of the likelihood column of MANY systems (the ready roots of a farm wave) that are on the
// device, in one call (like_moments_kernels.hpp has the four launches, like_moments.hpp the rule).  Everything is enqueued on the
// caller's stream; the host waits once, for one block of results.  Argument checks come before any device call.
#pragma once

#include "like_moments.hpp"
#include "like_moments_kernels.hpp"

namespace {

struct MomLayout {
    size_t off_segs = 0, off_tile0 = 0, off_sums = 0, off_part = 0, off_sys = 0, off_res = 0, total = 0;
    int64_t max_tiles = 0;
};

MomLayout mom_layout(int64_t nrows, int32_t nseg)
{
    MomLayout L;
    L.max_tiles = nrows / mce::kMomTileRows + nseg;
    const size_t S = (size_t)nseg, T = (size_t)L.max_tiles;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += prep_align(bytes); return at; };
    L.off_segs = take(S * sizeof(mce::MomSeg));
    L.off_tile0 = take(S * sizeof(int64_t));
    L.off_sums = take(T * mce::kMomTileSums * 8);
    L.off_part = take(T * 8);
    L.off_sys = take(S * mce::kMomSys * 8);
    L.off_res = take(S * mce_mom::kMomOut * 8);
    L.total = off;
    return L;
}

constexpr int32_t kMomMaxSegs = 1 << 20;

// the argument checks of both forms, and the tables
int mom_tables(const mce_moments_seg* segs, int32_t nseg, std::vector<mce::MomSeg>& table, std::vector<int64_t>& tile0, int64_t& nrows, int64_t& ntiles)
{
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kMomMaxSegs) return fail(MCE_ERR_INVALID, "like moments: %d segments (1 .. %d expected)", nseg, kMomMaxSegs);
    table.assign((size_t)nseg, mce::MomSeg{nullptr, nullptr, 0});
    tile0.assign((size_t)nseg, 0);
    nrows = 0;
    ntiles = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_moments_seg& g = segs[s];
        if (g.n < 0 || g.n > (int64_t)1 << 40 || (g.n > 0 && (!g.fs || !g.w)))
            return fail(MCE_ERR_INVALID, "like moments: segment %d has %lld rows at fs %s, w %s", s, (long long)g.n, g.fs ? "valid" : "null", g.w ? "valid" : "null");
        table[(size_t)s] = mce::MomSeg{g.fs, g.w, g.n};
        tile0[(size_t)s] = ntiles;
        ntiles += (g.n + mce::kMomTileRows - 1) / mce::kMomTileRows;
        nrows += g.n;
    }
    if (ntiles > 0x7fffffffLL) return fail(MCE_ERR_INVALID, "like moments: %lld rows in one call", (long long)nrows);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_like_moments_workspace_bytes(int64_t nrows_total, int32_t nseg)
{
    if (nrows_total < 0 || nseg < 1 || nseg > kMomMaxSegs) return 0;
    return mom_layout(nrows_total, nseg).total;
}

int mce_like_moments_dev(const mce_moments_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<MomSeg> table;
    std::vector<int64_t> tile0;
    int64_t nrows = 0, ntiles = 0;
    int rc = mom_tables(segs, nseg, table, tile0, nrows, ntiles);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    const MomLayout L = mom_layout(nrows, nseg);
    if (ws_bytes < L.total) return fail(MCE_ERR_WORKSPACE, "like moments: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    MomSeg* d_segs = prep_at<MomSeg>(ws, L.off_segs);
    int64_t* d_tile0 = prep_at<int64_t>(ws, L.off_tile0);
    double* d_sums = prep_at<double>(ws, L.off_sums);
    double* d_part = prep_at<double>(ws, L.off_part);
    double* d_sys = prep_at<double>(ws, L.off_sys);
    double* d_res = prep_at<double>(ws, L.off_res);

    MCE_HIP(hipMemcpyAsync(d_segs, table.data(), table.size() * sizeof(MomSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_tile0, tile0.data(), tile0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    const dim3 tb(kMomThreads);
    if (ntiles > 0) hipLaunchKernelGGL(mom_sum_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, d_segs, d_tile0, (int)nseg, d_sums);
    hipLaunchKernelGGL(mom_centre_kernel, dim3((unsigned)nseg), tb, 0, st, d_segs, d_tile0, d_sums, d_sys);
    if (ntiles > 0) hipLaunchKernelGGL(mom_var_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, d_segs, d_tile0, (int)nseg, d_sys, d_part);
    hipLaunchKernelGGL(mom_result_kernel, dim3((unsigned)nseg), tb, 0, st, d_segs, d_tile0, d_sys, d_part, d_res);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, d_res, (size_t)nseg * mce_mom::kMomOut * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    return MCE_OK;
}

int mce_like_moments_f64(const mce_moments_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<mce::MomSeg> table;
    std::vector<int64_t> tile0;
    int64_t nrows = 0, ntiles = 0;
    int rc = mom_tables(segs, nseg, table, tile0, nrows, ntiles);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    DevBuf cols, ws;
    MCE_HIP(cols.alloc((size_t)std::max<int64_t>(nrows, 1) * 2 * sizeof(double)));
    std::vector<mce_moments_seg> dsegs((size_t)nseg);
    int64_t at = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const int64_t n = segs[s].n;
        double* d_fs = cols.as<double>() + 2 * at;
        dsegs[(size_t)s] = mce_moments_seg{n > 0 ? d_fs : nullptr, n > 0 ? d_fs + n : nullptr, n};
        if (n > 0) {
            MCE_HIP(hipMemcpy(d_fs, segs[s].fs, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
            MCE_HIP(hipMemcpy(d_fs + n, segs[s].w, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
        }
        at += n;
    }
    const size_t wsb = mce_like_moments_workspace_bytes(nrows, nseg);
    MCE_HIP(ws.alloc(wsb));
    return mce_like_moments_dev(dsegs.data(), nseg, out, ws.p, wsb, nullptr);
}

}  // extern "C"
