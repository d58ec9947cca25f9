// capi_kde.hpp -- part of capi.hip (one translation unit): mce_kde_shift_out_doubles / mce_kde_shift_workspace_bytes /
// mce_kde_shift_dev / mce_kde_shift_f64: the leave-one-out kernel density sums of the whitened rows of MANY systems that are on the
// device, and the posterior mass above the density at a point, in one call (kde_kernels.hpp has the launches, kde_shift.hpp the rule).
// Everything is enqueued on the caller's stream; the host waits once, for one block of results.  Argument checks come before any device
// call.  Five launches, whatever the number of systems.
#pragma once

#include "capi_seg.hpp"
#include "kde_kernels.hpp"
#include "kde_shift.hpp"

namespace {

constexpr int32_t kKdeMaxSegs = 1 << 16;
constexpr int64_t kKdeMaxRows = 0x7fffffffLL;

// the workspace of a call: nrows_total rows in nseg segments, at most dmax columns
struct KdeWs {
    mce::KdeSeg* segs;
    int64_t* tile0;
    double *par, *z, *zn, *zp, *head, *sys, *partial, *mass, *res;
    size_t total;
    KdeWs(int64_t nrows_total, int32_t nseg, int32_t dmax, void* ws = nullptr)
    {
        const size_t S = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows_total, nseg), N = (size_t)nrows_total, D = (size_t)dmax;
        WsPlan P(ws);
        segs = P.take<mce::KdeSeg>(S);
        tile0 = P.take<int64_t>(S);
        par = P.take<double>(S * (D * D + 2 * D));
        z = P.take<double>(N * (size_t)mce_kde::kde_dpad(dmax));
        zn = P.take<double>(N);
        zp = P.take<double>(S * mce_kde::kKdeMaxDim);
        head = P.take<double>(T * mce::kKdeTileHead);
        sys = P.take<double>(S * mce::kKdeSys);
        partial = P.take<double>(N * mce_kde::kKdeMaxParts);
        mass = P.take<double>(T * mce::kKdeMass);
        res = P.take<double>(S * mce_kde::kKdeOut);
        total = P.total;
    }
};

struct KdeTables {
    std::vector<mce::KdeSeg> segs;
    mce_seg::SegTable tiles;
    std::vector<double> par;
    int32_t dmax = 1, pmax = 1;
};

// the argument checks of both forms, and the tables.  linv, mean and point are HOST arrays in both forms: they go into the parameter
// block here
int kde_tables(const mce_kde_seg* segs, int32_t nseg, KdeTables& T)
{
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kKdeMaxSegs) return fail(MCE_ERR_INVALID, "kde shift: %d segments (1 .. %d expected)", nseg, kKdeMaxSegs);
    T.segs.assign((size_t)nseg, mce::KdeSeg{});
    int64_t zoff = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_kde_seg& g = segs[s];
        if (g.d < 1 || g.d > mce_kde::kKdeMaxDim) return fail(MCE_ERR_INVALID, "kde shift: segment %d has d=%d (1 .. %d expected)", s, g.d, mce_kde::kKdeMaxDim);
        if (g.n < 0 || g.n > kKdeMaxRows || g.ld < g.d || (g.n > 0 && (!g.x || !g.w)) || !g.linv || !g.mean || !g.point)
            return fail(MCE_ERR_INVALID, "kde shift: segment %d has %lld rows, ld=%lld, d=%d at x %s, w %s, linv %s, mean %s, point %s", s, (long long)g.n,
                        (long long)g.ld, g.d, g.x ? "valid" : "null", g.w ? "valid" : "null", g.linv ? "valid" : "null", g.mean ? "valid" : "null",
                        g.point ? "valid" : "null");
        if (!(g.c > 0.0) || !(g.c - g.c == 0.0)) return fail(MCE_ERR_INVALID, "kde shift: segment %d has c=%g (positive and finite expected)", s, g.c);
        mce::KdeSeg& o = T.segs[(size_t)s];
        o.x = g.x; o.w = g.w; o.dens = g.dens; o.zout = g.zout; o.ld = g.ld; o.n = g.n; o.c = g.c; o.d = g.d; o.dpad = mce_kde::kde_dpad(g.d);
        o.row0 = T.tiles.nrows;
        o.zoff = zoff;
        o.par0 = (int64_t)T.par.size();
        zoff += g.n * o.dpad;
        const size_t D = (size_t)g.d;
        T.par.insert(T.par.end(), g.linv, g.linv + D * D);
        T.par.insert(T.par.end(), g.mean, g.mean + D);
        T.par.insert(T.par.end(), g.point, g.point + D);
        T.tiles.add(g.n);
        T.dmax = std::max(T.dmax, g.d);
        T.pmax = std::max(T.pmax, mce_kde::kde_nparts(g.n));
    }
    // (the sum kernel's grid: every tile's eight 64-row groups times the parts)
    if (!T.tiles.fits() || T.tiles.ntiles * mce::kKdeSubTiles * T.pmax > mce_seg::kSegMaxTiles)
        return fail(MCE_ERR_INVALID, "kde shift: %lld rows in one call", (long long)T.tiles.nrows);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_kde_shift_out_doubles(void) { return (size_t)mce_kde::kKdeOut; }

size_t mce_kde_shift_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t dmax)
{
    if (nrows_total < 0 || nseg < 1 || nseg > kKdeMaxSegs || dmax < 1 || dmax > mce_kde::kKdeMaxDim) return 0;
    return KdeWs(nrows_total, nseg, dmax).total;
}

int mce_kde_shift_dev(const mce_kde_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    KdeTables T;
    int rc = kde_tables(segs, nseg, T);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    const KdeWs W(T.tiles.nrows, nseg, T.dmax, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("kde shift", ws_bytes, W.total, T.segs, T.tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(W.par, T.par.data(), T.par.size() * sizeof(double), hipMemcpyHostToDevice, st));
    const dim3 tb(kKdeThreads);
    const int64_t ntiles = T.tiles.ntiles, nsum = ntiles * kKdeSubTiles * T.pmax;
    if (ntiles > 0) hipLaunchKernelGGL(kde_whiten_kernel, dim3((unsigned)ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, W.par, W.z, W.zn, W.zp, W.head);
    hipLaunchKernelGGL(kde_sys_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.head, W.sys);
    if (ntiles > 0) {
        hipLaunchKernelGGL(kde_sum_kernel, dim3((unsigned)nsum), tb, 0, st, W.segs, W.tile0, (int)nseg, (int)T.pmax, W.z, W.zn, W.partial);
        hipLaunchKernelGGL(kde_mass_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, W.segs, W.tile0, (int)nseg, W.sys, W.partial, W.mass);
    }
    hipLaunchKernelGGL(kde_result_kernel, dim3((unsigned)nseg), tb, 0, st, W.segs, W.tile0, W.sys, W.mass, W.res);
    return seg_dev_end(out, W.res, (size_t)nseg * mce_kde::kKdeOut, st);
}

int mce_kde_shift_f64(const mce_kde_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    KdeTables T;
    int rc = kde_tables(segs, nseg, T);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    // staged: the d measured columns and w; then, where asked for, the densities and the whitened rows, copied back at the end
    size_t bytes = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const size_t n = (size_t)segs[s].n, d = (size_t)segs[s].d;
        bytes += seg_stage_bytes(n * d * 8) + seg_stage_bytes(n * 8);
        if (segs[s].dens) bytes += seg_stage_bytes((n + 1) * 8);
        if (segs[s].zout) bytes += seg_stage_bytes(n * d * 8);
    }
    SegStage data;
    DevBuf ws;
    if ((rc = data.alloc(bytes)) != MCE_OK) return rc;
    std::vector<mce_kde_seg> dsegs(segs, segs + nseg);
    for (mce_kde_seg& g : dsegs) {
        if ((rc = data.put(g.x, (size_t)g.n, g.x, (size_t)g.d, (size_t)g.ld)) != MCE_OK || (rc = data.put(g.w, (size_t)g.n, g.w)) != MCE_OK) return rc;
        g.ld = g.d;
        if (g.dens) { g.dens = reinterpret_cast<double*>(data.at); data.at += seg_stage_bytes(((size_t)g.n + 1) * 8); }
        if (g.zout) { g.zout = reinterpret_cast<double*>(data.at); data.at += seg_stage_bytes((size_t)g.n * (size_t)g.d * 8); }
    }
    const size_t wsb = mce_kde_shift_workspace_bytes(T.tiles.nrows, nseg, T.dmax);
    MCE_HIP(ws.alloc(wsb));
    if ((rc = mce_kde_shift_dev(dsegs.data(), nseg, out, ws.p, wsb, nullptr)) != MCE_OK) return rc;
    for (int32_t s = 0; s < nseg; ++s) {
        const size_t n = (size_t)segs[s].n, d = (size_t)segs[s].d;
        if (segs[s].dens) MCE_HIP(hipMemcpy(segs[s].dens, dsegs[(size_t)s].dens, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (segs[s].zout && n > 0) MCE_HIP(hipMemcpy(segs[s].zout, dsegs[(size_t)s].zout, n * d * 8, hipMemcpyDeviceToHost));
    }
    return MCE_OK;
}

}  // extern "C"
