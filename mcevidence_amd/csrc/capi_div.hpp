// capi_div.hpp -- part of capi.hip (one translation unit): mce_div_whiten_* and mce_knn_div_*: the whitening of a chain in another
// chain's metric and the sums of the k-NN relative entropy with its delete-a-group jackknife from ONE pair of neighbour searches
// (knn_div_kernels.hpp has the passes, knn_div.hpp the rule, docs/design/knn_divergence.md the definition).  Argument checks come
// before any device call; the group ids are checked on the device; the stream is synchronised on return (the report and the count of
// short rows are small and the caller needs them to go on).
#pragma once

#include "knn_div.hpp"
#include "knn_div_kernels.hpp"

namespace {

int64_t div_blocks(int64_t n) { return std::max<int64_t>((n + mce::kRedThreads - 1) / mce::kRedThreads, 1); }

// the workspace of the whitening of n rows of d columns
struct DivWhitenWs {
    double *par, *partial, *report;
    size_t total;
    DivWhitenWs(int64_t n, int32_t d, void* ws = nullptr)
    {
        WsPlan P(ws);
        par = P.take<double>((size_t)d * (size_t)d + (size_t)d);
        partial = P.take<double>((size_t)div_blocks(n) * 3);
        report = P.take<double>(MCE_DIV_REPORT);
        total = P.total;
    }
};

// the workspace of nq queries against nP rows of P, G groups and K ranks
struct DivWs {
    double *partial, *mpart, *wp;
    int *flags, *cnt;
    int64_t* boff;
    int* bad;
    size_t total;
    int64_t nblocks, nblocksP;
    DivWs(int64_t nq, int64_t nP, int32_t G, int32_t K, void* ws = nullptr)
    {
        nblocks = div_blocks(nq);
        nblocksP = div_blocks(nP);
        WsPlan P(ws);
        partial = P.take<double>((size_t)nblocks * (size_t)(G + 1) * (size_t)K * 2);
        mpart = P.take<double>((size_t)nblocksP * (size_t)(G + 1));
        wp = P.take<double>((size_t)(G + 1));
        flags = P.take<int>((size_t)std::max<int64_t>(nq, 1));
        cnt = P.take<int>((size_t)nblocks);
        boff = P.take<int64_t>((size_t)nblocks);
        bad = P.take<int>(1);
        total = P.total;
    }
};

int div_whiten_check(int64_t ld, int64_t n, int32_t d)
{
    if (d < 1 || d > MCE_DIV_MAX_DIM) return fail(MCE_ERR_INVALID, "knn divergence: d=%d columns (1 .. %d expected)", d, MCE_DIV_MAX_DIM);
    if (n < 1 || ld < d) return fail(MCE_ERR_INVALID, "knn divergence: %lld rows of stride %lld for d=%d columns", (long long)n, (long long)ld, d);
    return MCE_OK;
}

int div_terms_check(int64_t nq, int32_t L, int64_t nP, int64_t nQ, int32_t G, int32_t K, int32_t d)
{
    if (G != 0 && (G < 2 || G > MCE_JACK_MAX_GROUPS)) return fail(MCE_ERR_INVALID, "knn divergence: G=%d groups (0, or 2 .. %d expected)", G, MCE_JACK_MAX_GROUPS);
    if (K < 1) return fail(MCE_ERR_INVALID, "knn divergence: K=%d ranks (1 .. %d expected)", K, MCE_DIV_MAX_K);
    if (K > MCE_DIV_MAX_K) return fail(MCE_ERR_K_RANGE, "knn divergence: K=%d ranks (1 .. %d expected)", K, MCE_DIV_MAX_K);
    if (L < K) return fail(MCE_ERR_INVALID, "knn divergence: lists of L=%d entries are shorter than the K=%d ranks of the sums", L, K);
    if (L > MCE_GENERIC_MAX_K) return fail(MCE_ERR_INVALID, "knn divergence: lists of L=%d entries (at most %d)", L, MCE_GENERIC_MAX_K);
    if (nq < 1 || nP < 1 || nQ < 1 || d < 1) return fail(MCE_ERR_INVALID, "knn divergence: invalid sizes nq=%lld nP=%lld nQ=%lld d=%d", (long long)nq, (long long)nP, (long long)nQ, d);
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_div_whiten_workspace_bytes(int64_t n, int32_t d)
{
    if (n < 1 || d < 1 || d > MCE_DIV_MAX_DIM) return 0;
    return DivWhitenWs(n, d).total;
}

int mce_div_whiten_dev(const double* d_x, int64_t ld, int64_t n, int32_t d, const double* linv, const double* mean, const double* d_w, double* d_z,
                       double* report, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!d_x || !linv || !mean || !d_w || !d_z || !report || !ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = div_whiten_check(ld, n, d);
    if (rc != MCE_OK) return rc;
    const DivWhitenWs lay(n, d, ws);
    if (ws_bytes < lay.total) return fail(MCE_ERR_WORKSPACE, "knn divergence: workspace of %zu bytes, %zu needed", ws_bytes, lay.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t D = (size_t)d;
    MCE_HIP(hipMemcpyAsync(lay.par, linv, D * D * sizeof(double), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(lay.par + D * D, mean, D * sizeof(double), hipMemcpyHostToDevice, st));
    const int64_t nb = div_blocks(n);
    hipLaunchKernelGGL(div_whiten_kernel, dim3((unsigned)nb), dim3(kRedThreads), (D * D + D) * sizeof(double), st, d_x, ld, n, (int)d, lay.par, d_w, d_z,
                       lay.partial);
    hipLaunchKernelGGL(div_report_kernel, dim3(1), dim3(kRedThreads), 0, st, lay.partial, nb, n, lay.report);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(report, lay.report, MCE_DIV_REPORT * sizeof(double), hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));
    return MCE_OK;
}

int mce_div_whiten_f64(const double* x, int64_t ld, int64_t n, int32_t d, const double* linv, const double* mean, const double* w, double* z,
                       double* report, int32_t device)
{
    if (!x || !linv || !mean || !w || !z || !report) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = div_whiten_check(ld, n, d);
    if (rc != MCE_OK) return rc;
    if ((rc = select_device(device)) != MCE_OK) return rc;
    DevBuf dX, dW, dZ, ws;
    const size_t wsb = mce_div_whiten_workspace_bytes(n, d);
    MCE_HIP(dX.alloc((size_t)n * ld * sizeof(double)));
    MCE_HIP(dW.alloc((size_t)n * sizeof(double)));
    MCE_HIP(dZ.alloc((size_t)n * d * sizeof(double)));
    MCE_HIP(ws.alloc(wsb));
    MCE_HIP(hipMemcpy(dX.p, x, (size_t)n * ld * sizeof(double), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dW.p, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    rc = mce_div_whiten_dev(dX.as<double>(), ld, n, d, linv, mean, dW.as<double>(), dZ.as<double>(), report, ws.p, wsb, nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpy(z, dZ.p, (size_t)n * d * sizeof(double), hipMemcpyDeviceToHost));
    return MCE_OK;
}

size_t mce_knn_div_workspace_bytes(int64_t nq, int64_t nP, int32_t G, int32_t K)
{
    if (nq < 1 || nP < 1 || (G != 0 && (G < 2 || G > MCE_JACK_MAX_GROUPS)) || K < 1 || K > MCE_DIV_MAX_K) return 0;
    return DivWs(nq, nP, G, K).total;
}

int mce_knn_div_terms_dev(const double* d_distP, const int64_t* d_idxP, const double* d_distQ, const int64_t* d_idxQ, int64_t nq, int32_t L,
                          const int64_t* d_qid, const int32_t* d_gq, const int32_t* d_grP, int64_t nP, const int32_t* d_grQ, int64_t nQ, int32_t G,
                          int32_t K, int32_t d, const double* d_aq, const double* d_aP, const double* d_bQ, double* d_sums, int64_t* d_short_rows,
                          int64_t* d_nshort, void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!d_distP || !d_idxP || !d_distQ || !d_idxQ || !d_aq || !d_aP || !d_bQ || !d_sums || !d_short_rows || !d_nshort || !ws)
        return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = div_terms_check(nq, L, nP, nQ, G, K, d);
    if (rc != MCE_OK) return rc;
    if (G > 0 && (!d_gq || !d_grP || !d_grQ)) return fail(MCE_ERR_INVALID, "null pointer argument");
    const DivWs lay(nq, nP, G, K, ws);
    if (ws_bytes < lay.total) return fail(MCE_ERR_WORKSPACE, "knn divergence: workspace of %zu bytes, %zu needed", ws_bytes, lay.total);
    if ((rc = prep_need_device()) != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)lay.nblocks), block(kRedThreads);

    if (G > 0) {
        MCE_HIP(zero_async(lay.bad, sizeof(int), st));
        hipLaunchKernelGGL(jack_check_groups_kernel, grid, block, 0, st, d_gq, nq, (int)G, lay.bad);
        hipLaunchKernelGGL(jack_check_groups_kernel, dim3((unsigned)lay.nblocksP), block, 0, st, d_grP, nP, (int)G, lay.bad);
        hipLaunchKernelGGL(jack_check_groups_kernel, dim3((unsigned)div_blocks(nQ)), block, 0, st, d_grQ, nQ, (int)G, lay.bad);
        MCE_HIP(hipGetLastError());
        int bad_h = 0;
        MCE_HIP(hipMemcpyAsync(&bad_h, lay.bad, sizeof(int), hipMemcpyDeviceToHost, st));
        MCE_HIP(hipStreamSynchronize(st));
        if (bad_h) return fail(MCE_ERR_INVALID, "knn divergence: a group id outside 0 .. %d", G - 1);
    }
    const int32_t* const gq = G > 0 ? d_gq : nullptr;
    const int32_t* const grP = G > 0 ? d_grP : nullptr;
    const int32_t* const grQ = G > 0 ? d_grQ : nullptr;

    // the weight of P and of its groups: per block, then over the blocks in jack_final_kernel's order
    hipLaunchKernelGGL(div_mass_kernel, dim3((unsigned)lay.nblocksP), block, 0, st, d_aP, grP, nP, (int)G, lay.mpart);
    hipLaunchKernelGGL(jack_final_kernel, dim3((unsigned)(G + 1)), block, 0, st, lay.mpart, lay.nblocksP, 1, 0, (int)(G + 1), lay.wp, (double*)nullptr);
    MCE_HIP(hipGetLastError());
    auto terms = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, st, d_distP, d_idxP, d_distQ, d_idxQ, nq, (int)L, d_qid, gq, grP, nP, grQ, nQ, (int)G, (int)K, (int)d, d_aq,
                           d_aP, d_bQ, (const double*)lay.wp, lay.partial, lay.flags, lay.cnt);
    };
    if (L <= kDivRegShort) terms(div_terms_kernel<kDivRegShort>);
    else if (L <= kDivRegL) terms(div_terms_kernel<kDivRegL>);
    else terms(div_terms_kernel<0>);
    MCE_HIP(hipGetLastError());
    // partial [nblocks][G + 1][2 K] -> d_sums [G + 1][K][2]: slot 0 first, then the groups
    hipLaunchKernelGGL(jack_final_kernel, dim3((unsigned)((G + 1) * K * 2)), block, 0, st, lay.partial, lay.nblocks, (int)(G + 1), 0, (int)(K * 2), d_sums,
                       d_sums + (size_t)K * 2);
    hipLaunchKernelGGL(jack_scan_kernel, dim3(1), block, 0, st, lay.cnt, lay.nblocks, lay.boff, d_nshort);
    hipLaunchKernelGGL(jack_compact_kernel, grid, block, 0, st, lay.flags, nq, d_qid, lay.boff, d_short_rows);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipStreamSynchronize(st));
    return MCE_OK;
}

int mce_knn_div_terms_f64(const double* distP, const int64_t* idxP, const double* distQ, const int64_t* idxQ, int64_t nq, int32_t L, const int64_t* qid,
                          const int32_t* gq, const int32_t* grP, int64_t nP, const int32_t* grQ, int64_t nQ, int32_t G, int32_t K, int32_t d,
                          const double* aq, const double* aP, const double* bQ, double* sums, int64_t* short_rows, int64_t* nshort, int32_t device)
{
    if (!distP || !idxP || !distQ || !idxQ || !aq || !aP || !bQ || !sums || !short_rows || !nshort) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = div_terms_check(nq, L, nP, nQ, G, K, d);
    if (rc != MCE_OK) return rc;
    if (G > 0) {
        if (!gq || !grP || !grQ) return fail(MCE_ERR_INVALID, "null pointer argument");
        for (int64_t i = 0; i < nq; ++i)
            if (gq[i] < 0 || gq[i] >= G) return fail(MCE_ERR_INVALID, "knn divergence: group id %d of query row %lld is outside 0 .. %d", gq[i], (long long)i, G - 1);
        for (int64_t i = 0; i < nP; ++i)
            if (grP[i] < 0 || grP[i] >= G) return fail(MCE_ERR_INVALID, "knn divergence: group id %d of row %lld of P is outside 0 .. %d", grP[i], (long long)i, G - 1);
        for (int64_t i = 0; i < nQ; ++i)
            if (grQ[i] < 0 || grQ[i] >= G) return fail(MCE_ERR_INVALID, "knn divergence: group id %d of row %lld of Q is outside 0 .. %d", grQ[i], (long long)i, G - 1);
    }
    if ((rc = select_device(device)) != MCE_OK) return rc;
    struct Up { const void* src; size_t bytes; DevBuf buf; };
    const size_t nl = (size_t)nq * (size_t)L;
    Up up[11] = {{distP, nl * 8, {}}, {idxP, nl * 8, {}}, {distQ, nl * 8, {}}, {idxQ, nl * 8, {}}, {qid, qid ? (size_t)nq * 8 : 0, {}},
                 {G > 0 ? gq : nullptr, G > 0 ? (size_t)nq * 4 : 0, {}}, {G > 0 ? grP : nullptr, G > 0 ? (size_t)nP * 4 : 0, {}},
                 {G > 0 ? grQ : nullptr, G > 0 ? (size_t)nQ * 4 : 0, {}}, {aq, (size_t)nq * 8, {}}, {aP, (size_t)nP * 8, {}}, {bQ, (size_t)nQ * 8, {}}};
    for (Up& u : up) {
        if (!u.src) continue;
        MCE_HIP(u.buf.alloc(u.bytes));
        MCE_HIP(hipMemcpy(u.buf.p, u.src, u.bytes, hipMemcpyHostToDevice));
    }
    DevBuf dS, dR, dN, ws;
    const size_t wsb = mce_knn_div_workspace_bytes(nq, nP, G, K), sb = (size_t)(G + 1) * K * 2 * sizeof(double);
    MCE_HIP(dS.alloc(sb));
    MCE_HIP(dR.alloc((size_t)nq * sizeof(int64_t)));
    MCE_HIP(dN.alloc(sizeof(int64_t)));
    MCE_HIP(ws.alloc(wsb));
    rc = mce_knn_div_terms_dev(up[0].buf.as<double>(), up[1].buf.as<int64_t>(), up[2].buf.as<double>(), up[3].buf.as<int64_t>(), nq, L,
                               up[4].buf.as<int64_t>(), up[5].buf.as<int32_t>(), up[6].buf.as<int32_t>(), nP, up[7].buf.as<int32_t>(), nQ, G, K, d,
                               up[8].buf.as<double>(), up[9].buf.as<double>(), up[10].buf.as<double>(), dS.as<double>(), dR.as<int64_t>(), dN.as<int64_t>(), ws.p,
                               wsb, nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpy(sums, dS.p, sb, hipMemcpyDeviceToHost));
    MCE_HIP(hipMemcpy(nshort, dN.p, sizeof(int64_t), hipMemcpyDeviceToHost));
    if (*nshort > 0) MCE_HIP(hipMemcpy(short_rows, dR.p,(size_t)*nshort * sizeof(int64_t), hipMemcpyDeviceToHost));
    return MCE_OK;
}

}  // extern "C"
