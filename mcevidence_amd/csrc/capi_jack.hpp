// capi_jack.hpp -- part of capi.hip (one translation unit): mce_jack_workspace_bytes / mce_jack_dotp_dev / mce_jack_dotp_f64: the
// leave-one-group-out sums of the evidence reduction from ONE neighbour search (jack_kernels.hpp has the passes, jack.hpp the rule,
// docs/design/jackknife.md the definition).  Argument checks come before any device call; the group ids are checked on the device and
// the stream is synchronised on return (the count of short rows is small and the caller needs it to go on).
#pragma once

#include "jack.hpp"
#include "jack_kernels.hpp"

namespace {

// the workspace of nq queries, G groups and kmax columns
struct JackWs {
    double* partial;
    int *flags, *cnt;
    int64_t* boff;
    int* bad;
    size_t total;
    int64_t nblocks;
    JackWs(int64_t nq, int32_t G, int32_t kmax, void* ws = nullptr)
    {
        nblocks = std::max<int64_t>((nq + mce::kRedThreads - 1) / mce::kRedThreads, 1);
        WsPlan P(ws);
        partial = P.take<double>((size_t)nblocks * (size_t)(G + 1) * (size_t)kmax);
        flags = P.take<int>((size_t)std::max<int64_t>(nq, 1));
        cnt = P.take<int>((size_t)nblocks);
        boff = P.take<int64_t>((size_t)nblocks);
        bad = P.take<int>(1);
        total = P.total;
    }
};

int jack_check_scalars(int64_t nq, int32_t L, int64_t nr, int32_t G, int32_t k0, int32_t kmax, int32_t d)
{
    if (G < 2 || G > MCE_JACK_MAX_GROUPS) return fail(MCE_ERR_INVALID, "jackknife: G=%d groups (2 .. %d expected)", G, MCE_JACK_MAX_GROUPS);
    if (k0 != 0 && k0 != 1) return fail(MCE_ERR_INVALID, "jackknife: k0 must be 0 (cross) or 1 (auto), got %d", k0);
    if (kmax <= k0 || kmax - k0 > MCE_MAX_K) return fail(MCE_ERR_INVALID, "jackknife: kmax=%d with k0=%d (1 .. %d columns expected)", kmax, k0, MCE_MAX_K);
    if (L < kmax - k0) return fail(MCE_ERR_INVALID, "jackknife: lists of L=%d entries are shorter than the K=%d neighbours of the sums", L, kmax - k0);
    if (L > MCE_GENERIC_MAX_K + 1) return fail(MCE_ERR_INVALID, "jackknife: lists of L=%d entries (at most %d)", L, MCE_GENERIC_MAX_K + 1);
    if (nq < 1 || nr < 1 || d < 1) return fail(MCE_ERR_INVALID, "jackknife: invalid sizes nq=%lld nr=%lld d=%d", (long long)nq, (long long)nr, d);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_jack_workspace_bytes(int64_t nq, int32_t G, int32_t kmax)
{
    if (nq < 1 || G < 2 || G > MCE_JACK_MAX_GROUPS || kmax < 1 || kmax > MCE_MAX_K + 1) return 0;
    return JackWs(nq, G, kmax).total;
}

int mce_jack_dotp_dev(const double* d_dist, const int64_t* d_idx, int64_t nq, int32_t L, const int64_t* d_qid, const int32_t* d_gq,
                      const int32_t* d_gr, int64_t nr, int32_t G, int32_t k0, int32_t kmax, int32_t d, const double* d_w, const double* d_fs,
                      double* d_dotp_groups, double* d_dotp_full, int64_t* d_short_rows, int64_t* d_nshort, void* ws, size_t ws_bytes,
                      void* stream)
{
    using namespace mce;
    if (!d_dist || !d_idx || !d_gq || !d_gr || !d_w || !d_fs || !d_dotp_groups || !d_dotp_full || !d_short_rows || !d_nshort || !ws)
        return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = jack_check_scalars(nq, L, nr, G, k0, kmax, d);
    if (rc != MCE_OK) return rc;
    const JackWs lay(nq, G, kmax, ws);
    if (ws_bytes < lay.total) return fail(MCE_ERR_WORKSPACE, "jackknife: workspace of %zu bytes, %zu needed", ws_bytes, lay.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);

    MCE_HIP(zero_async(lay.bad, sizeof(int), st));
    hipLaunchKernelGGL(jack_check_groups_kernel, dim3((unsigned)lay.nblocks), dim3(kRedThreads), 0, st, d_gq, nq, (int)G, lay.bad);
    hipLaunchKernelGGL(jack_check_groups_kernel, dim3((unsigned)((nr + kRedThreads - 1) / kRedThreads)), dim3(kRedThreads), 0, st, d_gr, nr, (int)G, lay.bad);
    MCE_HIP(hipGetLastError());
    int bad_h = 0;
    MCE_HIP(hipMemcpyAsync(&bad_h, lay.bad, sizeof(int), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    if (bad_h) return fail(MCE_ERR_INVALID, "jackknife: a group id outside 0 .. %d", G - 1);

    const dim3 grid((unsigned)lay.nblocks), block(kRedThreads);
    if (L <= kJackRegL)
        hipLaunchKernelGGL((jack_partial_kernel<true>), grid, block, 0, st, d_dist, d_idx, nq, (int)L, d_qid, d_gq, d_gr, nr, (int)G, (int)k0, (int)kmax,
                           (int)d, ln_unit_ball(d), d_w, d_fs, lay.partial, lay.flags, lay.cnt);
    else
        hipLaunchKernelGGL((jack_partial_kernel<false>), grid, block, 0, st, d_dist, d_idx, nq, (int)L, d_qid, d_gq, d_gr, nr, (int)G, (int)k0, (int)kmax,
                           (int)d, ln_unit_ball(d), d_w, d_fs, lay.partial, lay.flags, lay.cnt);
    MCE_HIP(hipGetLastError());
    hipLaunchKernelGGL(jack_final_kernel, dim3((unsigned)((G + 1) * kmax)), block, 0, st, lay.partial, lay.nblocks, (int)(G + 1), (int)k0, (int)kmax,
                       d_dotp_full, d_dotp_groups);
    hipLaunchKernelGGL(jack_scan_kernel, dim3(1), block, 0, st, lay.cnt, lay.nblocks, lay.boff, d_nshort);
    hipLaunchKernelGGL(jack_compact_kernel, grid, block, 0, st, lay.flags, nq, d_qid, lay.boff, d_short_rows);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipStreamSynchronize(st));
    return MCE_OK;
}

int mce_jack_dotp_f64(const double* dist, const int64_t* idx, int64_t nq, int32_t L, const int64_t* qid, const int32_t* gq, const int32_t* gr,
                      int64_t nr, int32_t G, int32_t k0, int32_t kmax, int32_t d, const double* w, const double* fs, double* dotp_groups,
                      double* dotp_full, int64_t* short_rows, int64_t* nshort, int32_t device)
{
    if (!dist || !idx || !gq || !gr || !w || !fs || !dotp_groups || !dotp_full || !short_rows || !nshort) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = jack_check_scalars(nq, L, nr, G, k0, kmax, d);
    if (rc != MCE_OK) return rc;
    for (int64_t i = 0; i < nq; ++i)
        if (gq[i] < 0 || gq[i] >= G) return fail(MCE_ERR_INVALID, "jackknife: group id %d of query row %lld is outside 0 .. %d", gq[i], (long long)i, G - 1);
    for (int64_t i = 0; i < nr; ++i)
        if (gr[i] < 0 || gr[i] >= G) return fail(MCE_ERR_INVALID, "jackknife: group id %d of reference row %lld is outside 0 .. %d", gr[i], (long long)i, G - 1);
    if ((rc = select_device(device)) != MCE_OK) return rc;
    DevBuf dD, dI, dQ, dGq, dGr, dW, dF, dOg, dOf, dS, dN, ws;
    const size_t wsb = mce_jack_workspace_bytes(nq, G, kmax);
    MCE_HIP(dD.alloc((size_t)nq * L * sizeof(double)));
    MCE_HIP(dI.alloc((size_t)nq * L * sizeof(int64_t)));
    if (qid) MCE_HIP(dQ.alloc((size_t)nq * sizeof(int64_t)));
    MCE_HIP(dGq.alloc((size_t)nq * sizeof(int32_t)));
    MCE_HIP(dGr.alloc((size_t)nr * sizeof(int32_t)));
    MCE_HIP(dW.alloc((size_t)nq * sizeof(double)));
    MCE_HIP(dF.alloc((size_t)nq * sizeof(double)));
    MCE_HIP(dOg.alloc((size_t)G * kmax * sizeof(double)));
    MCE_HIP(dOf.alloc((size_t)kmax * sizeof(double)));
    MCE_HIP(dS.alloc((size_t)nq * sizeof(int64_t)));
    MCE_HIP(dN.alloc(sizeof(int64_t)));
    MCE_HIP(ws.alloc(wsb));
    MCE_HIP(hipMemcpy(dD.p, dist, (size_t)nq * L * sizeof(double), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dI.p, idx, (size_t)nq * L * sizeof(int64_t), hipMemcpyHostToDevice));
    if (qid) MCE_HIP(hipMemcpy(dQ.p, qid, (size_t)nq * sizeof(int64_t), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dGq.p, gq, (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dGr.p, gr, (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dW.p, w, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dF.p, fs, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    rc = mce_jack_dotp_dev(dD.as<double>(), dI.as<int64_t>(), nq, L, qid ? dQ.as<int64_t>() : nullptr, dGq.as<int32_t>(), dGr.as<int32_t>(), nr, G, k0, kmax,
                           d, dW.as<double>(), dF.as<double>(), dOg.as<double>(), dOf.as<double>(), dS.as<int64_t>(), dN.as<int64_t>(), ws.p, wsb, nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpy(dotp_groups, dOg.p, (size_t)G * kmax * sizeof(double), hipMemcpyDeviceToHost));
    MCE_HIP(hipMemcpy(dotp_full, dOf.p, (size_t)kmax * sizeof(double), hipMemcpyDeviceToHost));
    MCE_HIP(hipMemcpy(nshort, dN.p, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (*nshort > 0) MCE_HIP(hipMemcpy(short_rows, dS.p, (size_t)*nshort * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MCE_OK;
}

}  // extern "C"
