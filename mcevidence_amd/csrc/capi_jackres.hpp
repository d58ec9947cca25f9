// capi_jackres.hpp -- part of capi.hip (one translation unit): mce_jack_groups_dev / mce_jack_leave_out_workspace_bytes /
// mce_jack_leave_out_dev / mce_jack_leave_out_f64: the bookkeeping of the delete-a-group jackknife for chains that stay on the device
// (the resident route and the farm): the group of every row, and the leave-one-group-out row counts, weight sums and likelihood moments
// of MANY systems in one call (jack_group_kernels.hpp has the launches, jack_groups.hpp the rule, docs/design/jackknife_resident.md the
// definition).  Everything is enqueued on the caller's stream; the host waits once.  Argument checks come before any device call; the
// group ids are checked on the device, in the first pass over them.
#pragma once

#include "capi_seg.hpp"
#include "jack_group_kernels.hpp"
#include "jack_groups.hpp"

namespace {

constexpr int32_t kJgMaxSegs = 1 << 20;

// the workspace of a call of nseg segments with nrows rows in all and at most Gmax groups.  res: one block per slot of every system,
// packed, and the flag of the group ids behind them
struct JgWs {
    mce::JgSeg* segs;
    int64_t* tile0;
    double *sums, *part, *sys, *res;
    size_t total;
    JgWs(int64_t nrows, int32_t nseg, int32_t Gmax, void* ws = nullptr)
    {
        const size_t S = (size_t)nseg, T = (size_t)mce_seg::seg_max_tiles(nrows, nseg), B = (size_t)Gmax + 1;
        WsPlan P(ws);
        segs = P.take<mce::JgSeg>(S);
        tile0 = P.take<int64_t>(S);
        sums = P.take<double>(T * B * mce::kJgTileSums);
        part = P.take<double>(T * B);
        sys = P.take<double>(S * B * mce::kJgSys);
        res = P.take<double>(S * B * mce_jg::kJgOut + 1);
        total = P.total;
    }
};

// the argument checks of both forms, and the tables
int jg_tables(const mce_jack_leave_out_seg* segs, int32_t nseg, std::vector<mce::JgSeg>& table, mce_seg::SegTable& tiles, int32_t& Gmax, int64_t& nslots_total)
{
    if (!segs) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nseg < 1 || nseg > kJgMaxSegs) return fail(MCE_ERR_INVALID, "jackknife leave-out: %d segments (1 .. %d expected)", nseg, kJgMaxSegs);
    table.assign((size_t)nseg, mce::JgSeg{nullptr, nullptr, nullptr, 0, 0, 0});
    nslots_total = 0;
    Gmax = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        const mce_jack_leave_out_seg& g = segs[s];
        if (g.G < 2 || g.G > MCE_JACK_MAX_GROUPS) return fail(MCE_ERR_INVALID, "jackknife: G=%d groups (2 .. %d expected)", g.G, MCE_JACK_MAX_GROUPS);
        if (g.n < 0 || g.n > (int64_t)1 << 40 || (g.n > 0 && (!g.w || !g.g)))
            return fail(MCE_ERR_INVALID, "jackknife leave-out: segment %d has %lld rows at w %s, g %s", s, (long long)g.n, g.w ? "valid" : "null", g.g ? "valid" : "null");
        table[(size_t)s] = mce::JgSeg{g.w, g.fs, g.g, g.n, g.G, (int32_t)nslots_total};
        tiles.add(g.n);
        nslots_total += g.G + 1;
        Gmax = std::max(Gmax, g.G);
    }
    if (!tiles.fits()) return fail(MCE_ERR_INVALID, "jackknife leave-out: %lld rows in one call", (long long)tiles.nrows);
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
    return JgWs(nrows_total, nseg, Gmax).total;
}

int mce_jack_leave_out_dev(const mce_jack_leave_out_seg* segs, int32_t nseg, double* out, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<JgSeg> table;
    mce_seg::SegTable tiles;
    int64_t nslots_total = 0;
    int32_t Gmax = 0;
    int rc = jg_tables(segs, nseg, table, tiles, Gmax, nslots_total);
    if (rc != MCE_OK) return rc;
    if (!ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    const JgWs W(tiles.nrows, nseg, Gmax, ws);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = seg_dev_begin("jackknife leave-out", ws_bytes, W.total, table, tiles.tile0, W.segs, W.tile0, st)) != MCE_OK) return rc;

    const size_t nres = (size_t)nslots_total * mce_jg::kJgOut;    // the flag of the group ids sits behind the blocks
    const int nslots = Gmax + 1;
    bool moments = false;
    for (const JgSeg& g : table) moments = moments || (g.fs != nullptr && g.n > 0);
    MCE_HIP(zero_async(W.res + nres, sizeof(double), st));
    const dim3 tb(kJgThreads), per_tile((unsigned)tiles.ntiles), per_slot((unsigned)nseg, (unsigned)nslots);
    if (tiles.ntiles > 0) hipLaunchKernelGGL(jg_sum_tile_kernel, per_tile, tb, 0, st, W.segs, W.tile0, (int)nseg, nslots, W.sums, W.res + nres);
    hipLaunchKernelGGL(jg_centre_kernel, per_slot, tb, 0, st, W.segs, W.tile0, nslots, W.sums, W.sys);
    if (tiles.ntiles > 0 && moments) hipLaunchKernelGGL(jg_var_tile_kernel, per_tile, tb, 0, st, W.segs, W.tile0, (int)nseg, nslots, W.sys, W.part);
    hipLaunchKernelGGL(jg_result_kernel, per_slot, tb, 0, st, W.segs, W.tile0, nslots, W.sys, W.part, W.res);
    std::vector<double> host(nres + 1);
    if ((rc = seg_dev_end(host.data(), W.res, nres + 1, st)) != MCE_OK) return rc;
    if (host[nres] != 0.0) return fail(MCE_ERR_INVALID, "jackknife: a group id outside 0 .. G - 1");
    std::copy(host.begin(), host.begin() + (ptrdiff_t)nres, out);
    return MCE_OK;
}

int mce_jack_leave_out_f64(const mce_jack_leave_out_seg* segs, int32_t nseg, double* out, int32_t device)
{
    if (!out) return fail(MCE_ERR_INVALID, "null pointer argument");
    std::vector<mce::JgSeg> table;
    mce_seg::SegTable tiles;
    int64_t nslots_total = 0;
    int32_t Gmax = 0;
    int rc = jg_tables(segs, nseg, table, tiles, Gmax, nslots_total);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    SegStage cols;
    DevBuf ws;
    size_t bytes = 0;
    for (int32_t s = 0; s < nseg; ++s) bytes += (size_t)segs[s].n * 2 * sizeof(double) + seg_stage_bytes((size_t)segs[s].n * sizeof(int32_t));
    if ((rc = cols.alloc(bytes)) != MCE_OK) return rc;
    std::vector<mce_jack_leave_out_seg> dsegs(segs, segs + nseg);
    for (mce_jack_leave_out_seg& g : dsegs)
        if ((rc = cols.put(g.w, (size_t)g.n, g.w)) != MCE_OK || (rc = cols.put(g.fs, (size_t)g.n, g.fs)) != MCE_OK || (rc = cols.put(g.g, (size_t)g.n, g.g)) != MCE_OK)
            return rc;
    const size_t wsb = mce_jack_leave_out_workspace_bytes(tiles.nrows, nseg, Gmax);
    MCE_HIP(ws.alloc(wsb));
    return mce_jack_leave_out_dev(dsegs.data(), nseg, out, ws.p, wsb, nullptr);
}

}  // extern "C"
