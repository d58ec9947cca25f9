// capi_jackres.hpp -- part of capi.hip (one translation unit): mce_jack_groups_dev / mce_jack_leave_out_workspace_bytes /
// mce_jack_leave_out_dev / mce_jack_leave_out_f64: the bookkeeping of the delete-a-group jackknife for chains that stay on the device
// (the resident route and the farm): the group of every row, and the leave-one-group-out row counts, weight sums and likelihood moments
// of MANY systems in one call (jack_group_kernels.hpp has the launches, jack_groups.hpp the rule, docs/design/jackknife_resident.md the
// definition).  Everything is enqueued on the caller's stream; the host waits once.  Argument checks come before any device call; the
// group ids are checked on the device, in the first pass over them.
#pragma once

#include "jack_group_kernels.hpp"
#include "jack_groups.hpp"

namespace {

constexpr int32_t kJgMaxSegs = 1 << 20;

struct JgLayout {
    size_t off_segs = 0, off_tile0 = 0, off_sums = 0, off_part = 0, off_sys = 0, off_res = 0, total = 0;
    int64_t max_tiles = 0;
};

// res: one block per slot of every system, packed, and the flag of the group ids behind them
JgLayout jg_layout(int64_t nrows, int32_t nseg, int32_t Gmax)
{
    JgLayout L;
    L.max_tiles = nrows / mce::kJgTileRows + nseg;
    const size_t S = (size_t)nseg, T = (size_t)L.max_tiles, B = (size_t)Gmax + 1;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += prep_align(bytes); return at; };
    L.off_segs = take(S * sizeof(mce::JgSeg));
    L.off_tile0 = take(S * sizeof(int64_t));
    L.off_sums = take(T * B * mce::kJgTileSums * 8);
    L.off_part = take(T * B * 8);
    L.off_sys = take(S * B * mce::kJgSys * 8);
    L.off_res = take((S * B * mce_jg::kJgOut + 1) * 8);
    L.total = off;
    return L;
}

// the argument checks of both forms, and the tables
int jg_tables(const mce_jack_leave_out_seg* segs, int32_t nseg, std::vector<mce::JgSeg>& table, std::vector<int64_t>& tile0, int64_t& nrows, int64_t& ntiles,
              int32_t& Gmax, int64_t& nslots_total)
{
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kJgMaxSegs) return fail(MCE_ERR_INVALID, "jackknife leave-out: %d segments (1 .. %d expected)", nseg, kJgMaxSegs);
    table.assign((size_t)nseg, mce::JgSeg{nullptr, nullptr, nullptr, 0, 0, 0});
    tile0.assign((size_t)nseg, 0);
    nrows = ntiles = nslots_total = 0;
    Gmax = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_jack_leave_out_seg& g = segs[s];
        if (g.G < 2 || g.G > MCE_JACK_MAX_GROUPS) return fail(MCE_ERR_INVALID, "jackknife: G=%d groups (2 .. %d expected)", g.G, MCE_JACK_MAX_GROUPS);
        if (g.n < 0 || g.n > (int64_t)1 << 40 || (g.n > 0 && (!g.w || !g.g)))
            return fail(MCE_ERR_INVALID, "jackknife leave-out: segment %d has %lld rows at w %s, g %s", s, (long long)g.n, g.w ? "valid" : "null", g.g ? "valid" : "null");
        table[(size_t)s] = mce::JgSeg{g.w, g.fs, g.g, g.n, g.G, (int32_t)nslots_total};
        tile0[(size_t)s] = ntiles;
        ntiles += (g.n + mce::kJgTileRows - 1) / mce::kJgTileRows;
        nrows += g.n;
        nslots_total += g.G + 1;
        Gmax = std::max(Gmax, g.G);
    }
    if (ntiles > 0x7fffffffLL) return fail(MCE_ERR_INVALID, "jackknife leave-out: %lld rows in one call", (long long)nrows);
    return MCE_OK;
}

}  // namespace

extern "C" {

int mce_jack_groups_dev(const mce_jack_groups_seg* segs, int32_t nseg, void* stream)
{
    using namespace mce;
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kJgMaxSegs) return fail(MCE_ERR_INVALID, "jackknife groups: %d segments (1 .. %d expected)", nseg, kJgMaxSegs);
    std::vector<JgGroupSeg> table((size_t)nseg);
    std::vector<int64_t> blk0((size_t)nseg, 0), firsts;
    std::vector<size_t> first_at((size_t)nseg, 0);
    int64_t nblk = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_jack_groups_seg& g = segs[s];
        if (g.by != mce_jg::kJgBlocks && g.by != mce_jg::kJgChains) return fail(MCE_ERR_INVALID, "jackknife groups: by=%d (0: blocks, 1: chains)", g.by);
        if (g.G < 2 || g.G > MCE_JACK_MAX_GROUPS) return fail(MCE_ERR_INVALID, "jackknife: G=%d groups (2 .. %d expected)", g.G, MCE_JACK_MAX_GROUPS);
        if (g.n < 0 || g.n > (int64_t)1 << 40 || g.N < 0 || g.N > (int64_t)1 << 40 || (g.n > 0 && (!g.out || g.N < 1)))
            return fail(MCE_ERR_INVALID, "jackknife groups: segment %d has %lld rows of a sample of %lld, out %s", s, (long long)g.n, (long long)g.N,
                        g.out ? "valid" : "null");
        if (g.by == mce_jg::kJgChains) {
            if (!g.part_first || g.nparts != g.G)
                return fail(MCE_ERR_INVALID, "jackknife groups: segment %d has %lld parts for G=%d chains", s, (long long)g.nparts, g.G);
            for (int64_t p = 0; p < g.nparts; ++p)
                if (g.part_first[p] < 0 || (p == 0 && g.part_first[p] != 0) || (p > 0 && g.part_first[p] < g.part_first[p - 1]))
                    return fail(MCE_ERR_INVALID, "jackknife groups: the parts' first rows of segment %d do not start at 0 or decrease", s);
            first_at[(size_t)s] = firsts.size();
            firsts.insert(firsts.end(), g.part_first, g.part_first + g.nparts);
        }
        table[(size_t)s] = JgGroupSeg{g.rows, g.src, nullptr, g.by == mce_jg::kJgChains ? g.nparts : 0, g.n, g.N, g.G, g.by, g.out};
        blk0[(size_t)s] = nblk;
        nblk += (g.n + kJgThreads - 1) / kJgThreads;
    }
    if (nblk > 0x7fffffffLL) return fail(MCE_ERR_INVALID, "jackknife groups: too many rows in one call");
    if (nblk == 0) return MCE_OK;
    int rc = prep_need_device();
    if (rc != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the tables: segments | first blocks | the parts' first rows
    const size_t b_segs = prep_align(table.size() * sizeof(JgGroupSeg)), b_blk = prep_align(blk0.size() * sizeof(int64_t));
    DevBuf tab;
    MCE_HIP(tab.alloc(b_segs + b_blk + std::max<size_t>(firsts.size(), 1) * sizeof(int64_t)));
    JgGroupSeg* d_segs = prep_at<JgGroupSeg>(tab.p, 0);
    int64_t* d_blk0 = prep_at<int64_t>(tab.p, b_segs);
    int64_t* d_firsts = prep_at<int64_t>(tab.p, b_segs + b_blk);
    for (int32_t s = 0; s < nseg; ++s)
        if (table[(size_t)s].by == mce_jg::kJgChains) table[(size_t)s].part_first = d_firsts + first_at[(size_t)s];
    MCE_HIP(hipMemcpyAsync(d_segs, table.data(), table.size() * sizeof(JgGroupSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_blk0, blk0.data(), blk0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (!firsts.empty()) MCE_HIP(hipMemcpyAsync(d_firsts, firsts.data(), firsts.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(jg_groups_kernel, dim3((unsigned)nblk), dim3(kJgThreads), 0, st, d_segs, d_blk0, (int)nseg);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait: the tables go out of scope here
    return MCE_OK;
}

size_t mce_jack_leave_out_workspace_bytes(int64_t nrows_total, int32_t nseg, int32_t Gmax)
{
    if (nrows_total < 0 || nseg < 1 || nseg > kJgMaxSegs || Gmax < 2 || Gmax > MCE_JACK_MAX_GROUPS) return 0;
    return jg_layout(nrows_total, nseg, Gmax).total;
}

int mce_jack_leave_out_dev(const mce_jack_leave_out_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<JgSeg> table;
    std::vector<int64_t> tile0;
    int64_t nrows = 0, ntiles = 0, nslots_total = 0;
    int32_t Gmax = 0;
    int rc = jg_tables(segs, nseg, table, tile0, nrows, ntiles, Gmax, nslots_total);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    const JgLayout L = jg_layout(nrows, nseg, Gmax);
    if (ws_bytes < L.total) return fail(MCE_ERR_WORKSPACE, "jackknife leave-out: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    JgSeg* d_segs = prep_at<JgSeg>(ws, L.off_segs);
    int64_t* d_tile0 = prep_at<int64_t>(ws, L.off_tile0);
    double* d_sums = prep_at<double>(ws, L.off_sums);
    double* d_part = prep_at<double>(ws, L.off_part);
    double* d_sys = prep_at<double>(ws, L.off_sys);
    double* d_res = prep_at<double>(ws, L.off_res);
    const size_t nres = (size_t)nslots_total * mce_jg::kJgOut;    // the flag of the group ids sits behind the blocks
    const int nslots = Gmax + 1;
    bool moments = false;
    for (const JgSeg& g : table) moments = moments || (g.fs != nullptr && g.n > 0);

    MCE_HIP(hipMemcpyAsync(d_segs, table.data(), table.size() * sizeof(JgSeg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_tile0, tile0.data(), tile0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    MCE_HIP(zero_async(d_res + nres, sizeof(double), st));
    const dim3 tb(kJgThreads), per_slot((unsigned)nseg, (unsigned)nslots);
    if (ntiles > 0) hipLaunchKernelGGL(jg_sum_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, d_segs, d_tile0, (int)nseg, nslots, d_sums, d_res + nres);
    hipLaunchKernelGGL(jg_centre_kernel, per_slot, tb, 0, st, d_segs, d_tile0, nslots, d_sums, d_sys);
    if (ntiles > 0 && moments) hipLaunchKernelGGL(jg_var_tile_kernel, dim3((unsigned)ntiles), tb, 0, st, d_segs, d_tile0, (int)nseg, nslots, d_sys, d_part);
    hipLaunchKernelGGL(jg_result_kernel, per_slot, tb, 0, st, d_segs, d_tile0, nslots, d_sys, d_part, d_res);
    MCE_HIP(hipGetLastError());
    std::vector<double> host(nres + 1);
    MCE_HIP(hipMemcpyAsync(host.data(), d_res, (nres + 1) * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    if (host[nres] != 0.0) return fail(MCE_ERR_INVALID, "jackknife: a group id outside 0 .. G - 1");
    std::copy(host.begin(), host.begin() + (ptrdiff_t)nres, out);
    return MCE_OK;
}

int mce_jack_leave_out_f64(const mce_jack_leave_out_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<mce::JgSeg> table;
    std::vector<int64_t> tile0;
    int64_t nrows = 0, ntiles = 0, nslots_total = 0;
    int32_t Gmax = 0;
    int rc = jg_tables(segs, nseg, table, tile0, nrows, ntiles, Gmax, nslots_total);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    DevBuf cols, ids, ws;
    MCE_HIP(cols.alloc((size_t)std::max<int64_t>(nrows, 1) * 2 * sizeof(double)));
    MCE_HIP(ids.alloc((size_t)std::max<int64_t>(nrows, 1) * sizeof(int32_t)));
    std::vector<mce_jack_leave_out_seg> dsegs((size_t)nseg);
    int64_t at = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const int64_t n = segs[s].n;
        double* d_w = cols.as<double>() + 2 * at;
        int32_t* d_g = ids.as<int32_t>() + at;
        dsegs[(size_t)s] = mce_jack_leave_out_seg{n > 0 ? d_w : nullptr, (n > 0 && segs[s].fs) ? d_w + n : nullptr, n > 0 ? d_g : nullptr, n, segs[s].G};
        if (n > 0) {
            MCE_HIP(hipMemcpy(d_w, segs[s].w, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
            if (segs[s].fs) MCE_HIP(hipMemcpy(d_w + n, segs[s].fs, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
            MCE_HIP(hipMemcpy(d_g, segs[s].g, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        at += n;
    }
    const size_t wsb = mce_jack_leave_out_workspace_bytes(nrows, nseg, Gmax);
    MCE_HIP(ws.alloc(wsb));
    return mce_jack_leave_out_dev(dsegs.data(), nseg, out, ws.p, wsb, nullptr);
}

}  // extern "C"
