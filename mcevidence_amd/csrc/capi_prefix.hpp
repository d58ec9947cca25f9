// capi_prefix.hpp -- part of capi.hip: the convergence batches of the evidence feed (mce_evidence_feed_prefix_f64 and its
// device-pointer twin).  Entry b is the feed of the FIRST prefix[b] rows of S1 (reference MCEvidence.py:1034-1131 with
// brange / nbatch): one upload, the B shifts max(logl[0 : p_b]) in one pass (prefix_kernels.hpp), and then
//   cov_mode 0, auto    one covariance of ALL rows, one eigen-system, one whitening in place; per distinct prefix the
//                       likelihood terms into one scratch and a search of the first p_b rows of the shared buffer
//   cov_mode 1, auto    the B covariances of the raw prefixes enqueued into their own slots, ONE synchronisation, B Jacobi
//                       solves on the host; per distinct prefix an out-of-place whitening into a scratch and its search
//   cov_mode 0, cross   one whitening of s1 U s2, ONE search of S1[:p_max] against all of S2 that leaves its distances, and the
//                       B reductions from them (every batch searches all of s2: reference :1075)
// on one stream.  The host waits twice whatever B is: for the covariances (the eigen-solves are the host's), and at the end.
// With the device eigen-solver (mce_options.eig_mode 2, capi_eig.hpp) all the systems are solved in ONE launch behind the
// covariances, every whitening reads its own slot of the solver's output, and the host waits once, at the end.
// The arena and the pinned block are feed_layout.hpp's (PrefixArena, PrefixPinned); the checks, the copy in, the solves, the device
// solver's results and the certificate are the feed's (capi_feed.hpp).
#pragma once
namespace {

struct PrefixJob {
    const double *S1 = nullptr, *S2 = nullptr, *w = nullptr, *logl = nullptr;
    int64_t n1 = 0, ld1 = 0, n2 = 0, ld2 = 0, ntot = 0, nr = 0, pmax = 0;
    int d = 0, cov_mode = 0, kmax = 0, k0 = 1, K = 0, B = 0;
    const int64_t* prefix = nullptr;
    bool src_device = false;
    // distinct prefixes, in order: first[i] = the first entry b of the i-th distinct size; every entry's distinct index
    std::vector<int> first, which;
    std::vector<Plan> plans;            // per distinct prefix (auto); one plan (cross)
    std::vector<int> nverify;           // rows re-checked per search
    int nsearch = 0, nsys = 0;
    mce_feed::PrefixSizes z;            // z.dev_eig: the eigen-systems on the device: stage B is skipped
    mce_feed::PrefixArena a;
    mce_feed::PrefixPinned h;

    bool cross() const { return S2 != nullptr; }
    int64_t size_of(int i) const { return prefix[first[i]]; }
    FeedIn in() const { return FeedIn{S1, S2, w, logl, n1, ld1, n2, ld2, d}; }
    // a failure of distinct prefix i, in the caller's words
    int fail_at(int rc, int i) const
    {
        const std::string msg = g_err;
        return fail(rc, "prefix %d (%lld rows): %s", first[i], (long long)size_of(i), msg.c_str());
    }
};

// argument checks + sizes; no device work
int prefix_plan(PrefixJob& j, const double* dotp, const double* loglmax, const double* jacobian)
{
    if (!j.S1 || !j.w || !j.logl || !j.prefix || !dotp || !loglmax || !jacobian) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (j.B < 1 || j.B > MCE_MAX_PREFIX) return fail(MCE_ERR_INVALID, "nprefix=%d must lie in 1..%d", j.B, MCE_MAX_PREFIX);
    int rc = feed_check(j.in(), j.cov_mode, j.kmax, true, j.k0, j.K);
    if (rc != MCE_OK) return rc;
    for (int b = 0; b < j.B; ++b) {
        const int64_t p = j.prefix[b];
        if (b > 0 && p < j.prefix[b - 1]) return fail(MCE_ERR_INVALID, "prefix %d (%lld rows) is smaller than prefix %d (%lld rows): sizes must not decrease", b, (long long)p, b - 1, (long long)j.prefix[b - 1]);
        if (p > j.n1) return fail(MCE_ERR_INVALID, "prefix %d (%lld rows) exceeds n1=%lld", b, (long long)p, (long long)j.n1);
        if (p < (int64_t)j.kmax + 1) return fail(MCE_ERR_INVALID, "prefix %d (%lld rows) is smaller than kmax + 1 = %d", b, (long long)p, j.kmax + 1);
    }
    static_assert(MCE_MAX_PREFIX == mce::kMaxPrefix, "prefix_max_kernel keeps the sizes in LDS");
    j.pmax = j.prefix[j.B - 1];
    j.nr = j.S2 ? j.n2 : 0;
    j.ntot = j.n1 + (j.S2 ? j.n2 : 0);
    j.which.assign(j.B, 0);
    for (int b = 0; b < j.B; ++b) {
        if (b == 0 || j.prefix[b] != j.prefix[b - 1]) j.first.push_back(b);
        j.which[b] = (int)j.first.size() - 1;
    }
    const int nd = (int)j.first.size();
    j.nsearch = j.cross() ? 1 : nd;
    j.nsys = j.cov_mode == 1 ? nd : 1;
    j.plans.resize(j.nsearch);
    j.nverify.assign(j.nsearch, 0);
    SameSetHint hint(!j.cross());          // as in feed_plan
    mce_feed::PrefixSizes& z = j.z;
    for (int i = 0; i < j.nsearch; ++i) {
        const int64_t nq = j.cross() ? j.pmax : j.size_of(i), nref = j.cross() ? j.n2 : nq;
        rc = make_plan(nq, nref, j.d, j.K, j.k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, j.plans[i]);
        if (rc != MCE_OK) return rc;
        z.search_ws_bytes = std::max(z.search_ws_bytes, j.plans[i].total + dotp_ws_bytes(nq, j.kmax));      // (plans need not grow with p: the maximum)
        if (j.d <= mce::kVerifyMaxDim && j.K <= mce::kVerifyMaxK) j.nverify[i] = (int)std::min<int64_t>(eff_verify(j.plans[i].filter(), nq), nq);
        if (j.nverify[i] > 0) {
            z.vrows = std::max(z.vrows, nq);
            z.verify_ws_bytes = std::max(z.verify_ws_bytes, mce_verify_workspace_bytes(j.nverify[i], j.K));
        }
    }
    if (j.cross()) z.vrows = j.pmax;          // the reductions read the search's distances
    z.n1 = j.n1; z.ntot = j.ntot; z.pmax = j.pmax; z.d = j.d; z.kmax = j.kmax; z.K = j.K; z.B = j.B;
    z.nsearch = j.nsearch; z.nsys = j.nsys;
    z.nblk_max = (int)((j.pmax + mce::kPrefixMaxRows - 1) / mce::kPrefixMaxRows);
    z.nblk_dotp = (int)((j.pmax + mce::kPrefixThreads - 1) / mce::kPrefixThreads);
    z.own_systems = j.cov_mode == 1;
    z.cross = j.cross();
    z.part_doubles = feed_part_doubles(j.d);
    z.dev_eig = eff_eig_mode() == 2;
    z.stat_ints = mce_eig::kStatInts;
    j.a = mce_feed::PrefixArena(z);
    j.h = mce_feed::PrefixPinned(z);
    return MCE_OK;
}

// upload, the B shifts, the covariance(s); everything enqueued on st, the small results on their way to the pinned arena
int prefix_stage_a(PrefixJob& j, hipStream_t st)
{
    const mce_feed::PrefixArena& a = j.a;
    const int d = j.d;
    int rc = feed_copy_in(j.in(), a.S1, a.S2, a.W, a.L, j.src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st, nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(a.P, j.prefix, (size_t)j.B * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mce::prefix_max_kernel, dim3((unsigned)j.z.nblk_max), dim3(mce::kPrefixThreads), 0, st, a.L, a.P, j.B, a.blk, j.z.nblk_max);
    MCE_HIP(hipGetLastError());
    hipLaunchKernelGGL(mce::prefix_max_final_kernel, dim3(1), dim3(mce::kPrefixThreads), 0, st, a.blk, a.P, j.B, j.z.nblk_max, a.lmax);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(j.h.lmax, a.lmax, (size_t)j.B * sizeof(double), hipMemcpyDeviceToHost, st));
    // "all": ONE eigen-system from every row of s1 U s2, whatever the prefix (reference :1034-1037); "single": each prefix's own
    for (int i = 0; i < j.nsys; ++i) {
        rc = launch_covariance(a.S1, j.cov_mode == 0 ? j.ntot : j.size_of(i), d, a.part, a.mean3, a.cov_at(i), st);
        if (rc != MCE_OK) return rc;
    }
    if (j.z.dev_eig) return launch_eig(a.cov, d, j.nsys, a.eig.evec, a.eig.scale, a.eig.back.lam, a.eig.back.status, st);      // all systems, one launch
    MCE_HIP(hipMemcpyAsync(j.h.sys, a.cov, (size_t)j.nsys * d * d * sizeof(double), hipMemcpyDeviceToHost, st));
    return MCE_OK;
}

// the eigen-systems' Jacobians, jac[i] of system i: from the host's solves (stage B; the eigenvectors replace the covariances they
// were solved from), or from the device solver's results once the call has finished.  The first system that failed names the error.
int prefix_systems(PrefixJob& j, std::vector<double>& jac)
{
    std::vector<std::vector<double>> lam;
    int at = 0;
    const int rc = j.z.dev_eig ? feed_eig_results(j.h.eig, j.nsys, g_eig_stats, at)
                               : feed_solve_host(j.nsys, j.d, j.h.sys, j.h.sys, j.h.scale, lam, g_eig_stats, at);
    if (rc != MCE_OK) return j.cov_mode == 0 ? rc : j.fail_at(rc, at);
    jac.assign(j.nsys, 0.0);
    for (int i = 0; i < j.nsys; ++i) jac[i] = feed_jacobian(j.z.dev_eig ? std::vector<double>(j.h.eig.lam_at(i), j.h.eig.lam_at(i) + j.d) : lam[i]);
    return MCE_OK;
}

// the whitening of system i's rows: from the host's solve (uploaded here) or from the device solver's slot, with its status
int prefix_whiten(PrefixJob& j, int i, int64_t n, double* out, hipStream_t st)
{
    const mce_feed::PrefixArena& a = j.a;
    if (j.z.dev_eig) return launch_whiten(a.S1, n, j.d, a.eig.evec_at(i), a.eig.scale_at(i), out, st, a.eig.back.status_at(i));
    MCE_HIP(hipMemcpyAsync(a.evec, j.h.sys_at(i), (size_t)j.d * j.d * sizeof(double), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(a.scale, j.h.scale_at(i), (size_t)j.d * sizeof(double), hipMemcpyHostToDevice, st));
    return launch_whiten(a.S1, n, j.d, a.evec, a.scale, out, st);
}

int prefix_fs(PrefixJob& j, int64_t p, int b, hipStream_t st)
{
    hipLaunchKernelGGL(mce::prefix_fs_kernel, dim3((unsigned)((p + mce::kPrefixThreads - 1) / mce::kPrefixThreads)), dim3(mce::kPrefixThreads), 0, st,
                       j.a.L, p, j.a.lmax + b, j.a.F);
    MCE_HIP(hipGetLastError());
    return MCE_OK;
}

// mce_options.verify, as in feed_stage_c: re-check a sample of the rows of search i
int prefix_verify(PrefixJob& j, int i, const double* X, int64_t nq, const double* Y, int64_t nref, hipStream_t st)
{
    if (j.nverify[i] <= 0) return MCE_OK;
    return feed_verify_enqueue(X, nq, Y, nref, j.d, j.K, j.k0, j.a.vdist, j.nverify[i], i, j.a.vres + 2 * i, j.a.vws, j.h.verify + 2 * i, st);
}

// whitening, the searches and the reductions
int prefix_stage_c(PrefixJob& j, hipStream_t st)
{
    const mce_feed::PrefixArena& a = j.a;
    const size_t wsb = j.z.search_ws_bytes;
    int rc = whiten_attr_once();
    if (rc != MCE_OK) return rc;
    const int d = j.d;
    if (j.cov_mode == 0) {
        rc = prefix_whiten(j, 0, j.ntot, a.S1, st);
        if (rc != MCE_OK) return rc;
    }
    SameSetHint hint(!j.cross());          // as in prefix_plan: the workspace was sized with it
    if (j.cross()) {
        // ONE search of the longest prefix against all of s2; its distances serve every batch
        rc = prefix_fs(j, j.pmax, j.B - 1, st);
        if (rc != MCE_OK) return rc;
        rc = mce_knn_dotp_f64_dev(a.S1, j.pmax, a.S2, j.n2, d, j.kmax, 0, 0, a.W, a.F, a.O, a.vdist, a.ws, wsb, st);
        if (rc != MCE_OK) return rc;
        hipLaunchKernelGGL(mce::prefix_dotp_kernel, dim3((unsigned)j.z.nblk_dotp, (unsigned)j.B), dim3(mce::kPrefixThreads), 0, st, a.vdist, j.K, j.kmax, d,
                           ln_unit_ball(d), a.W, a.L, a.lmax, a.P, a.dpart);
        MCE_HIP(hipGetLastError());
        hipLaunchKernelGGL(mce::prefix_dotp_final_kernel, dim3((unsigned)j.kmax, (unsigned)j.B), dim3(mce::kPrefixThreads), 0, st, a.dpart,
                           (int64_t)j.z.nblk_dotp, j.kmax, a.O);
        MCE_HIP(hipGetLastError());
        rc = prefix_verify(j, 0, a.S1, j.pmax, a.S2, j.n2, st);
        if (rc != MCE_OK) return rc;
    } else {
        for (int i = 0; i < j.nsearch; ++i) {
            const int b = j.first[i];
            const int64_t p = j.size_of(i);
            const double* X = a.S1;
            if (j.cov_mode == 1) {          // the prefix's own system: out of place, the raw rows serve the next prefix
                rc = prefix_whiten(j, i, p, a.X, st);
                if (rc != MCE_OK) return rc;
                X = a.X;
            }
            rc = prefix_fs(j, p, b, st);
            if (rc != MCE_OK) return rc;
            rc = mce_knn_dotp_f64_dev(X, p, X, p, d, j.kmax, 1, 0, a.W, a.F, a.O + (size_t)b * j.kmax, j.nverify[i] > 0 ? a.vdist : nullptr, a.ws, wsb, st);
            if (rc == MCE_OK) rc = prefix_verify(j, i, X, p, X, p, st);
            if (rc != MCE_OK) return j.fail_at(rc, i);
        }
    }
    MCE_HIP(hipMemcpyAsync(j.h.dotp, a.O, (size_t)j.B * j.kmax * sizeof(double), hipMemcpyDeviceToHost, st));
    if (j.z.dev_eig) MCE_HIP(hipMemcpyAsync(j.h.eig.lam, a.eig.back.lam, a.eig.back.bytes, hipMemcpyDeviceToHost, st));
    return MCE_OK;
}

int prefix_stage_d(PrefixJob& j, const std::vector<double>& jac, double* dotp, double* loglmax, double* jacobian)
{
    for (int b = 0; b < j.B; ++b) {
        // equal prefixes were computed once: the first of them holds the sums (cross: every entry was reduced)
        const int src = j.cross() ? b : j.first[j.which[b]];
        std::copy(j.h.dotp + (size_t)src * j.kmax, j.h.dotp + (size_t)(src + 1) * j.kmax, dotp + (size_t)b * j.kmax);
        loglmax[b] = j.h.lmax[b];
        jacobian[b] = jac[j.cov_mode == 1 ? j.which[b] : 0];
    }
    int checked = 0;
    for (int i = 0; i < j.nsearch; ++i) {
        if (j.nverify[i] <= 0) continue;
        const int* res = j.h.verify + 2 * i;
        checked += res[0];
        if (res[1] != 0) {
            g_last_verify_rows.store(checked);
            const int b = j.cross() ? j.B - 1 : j.first[i];
            return fail(MCE_ERR_VERIFY, "prefix %d (%lld rows): k-NN re-check failed: %d of %d sampled query rows have a neighbour list that an exact fp64 scan of "
                        "all %lld reference rows contradicts", b, (long long)j.prefix[b], res[1], res[0], (long long)(j.cross() ? j.n2 : j.prefix[b]));
        }
    }
    g_last_verify_rows.store(checked);          // rows re-checked over all searches of the call
    return MCE_OK;
}

int feed_prefix_impl(bool src_device, const double* S1, int64_t n1, int64_t ld1, const double* S2, int64_t n2, int64_t ld2, int32_t d, int32_t cov_mode,
                     int32_t kmax, const double* w, const double* logl, const int64_t* prefix, int32_t nprefix, double* dotp, double* loglmax,
                     double* jacobian, int32_t device)
{
    g_eig_stats = EigStats();
    PrefixJob j;
    j.S1 = S1; j.n1 = n1; j.ld1 = ld1;
    j.S2 = S2; j.n2 = S2 ? n2 : 0; j.ld2 = S2 ? ld2 : 0;
    j.d = d; j.cov_mode = cov_mode; j.kmax = kmax;
    j.w = w; j.logl = logl; j.prefix = prefix; j.B = nprefix;
    j.src_device = src_device;
    int rc = prefix_plan(j, dotp, loglmax, jacobian);
    if (rc != MCE_OK) return rc;
    rc = select_device(device);
    if (rc != MCE_OK) return rc;
    DevBuf arena;
    Quiesce quiesce;
    MCE_HIP(arena.alloc(j.a.total));
    MCE_HIP(g_pinned.reserve(j.h.total));
    j.a = mce_feed::PrefixArena(j.z, arena.p);
    j.h = mce_feed::PrefixPinned(j.z, g_pinned.p);
    hipStream_t st = nullptr;
    std::vector<double> jac;
    rc = prefix_stage_a(j, st);
    if (rc != MCE_OK) return rc;
    if (!j.z.dev_eig) {
        MCE_HIP(hipStreamSynchronize(st));
        rc = prefix_systems(j, jac);
        if (rc != MCE_OK) return rc;
    }
    rc = prefix_stage_c(j, st);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipStreamSynchronize(st));
    quiesce.armed = false;
    if (j.z.dev_eig) {          // the solves' status first: a failed system's searches ran on placeholder rows
        rc = prefix_systems(j, jac);
        if (rc != MCE_OK) return rc;
    }
    return prefix_stage_d(j, jac, dotp, loglmax, jacobian);
}

}  // namespace

extern "C" {

int mce_evidence_feed_prefix_f64(const double* S1, int64_t n1, int64_t ld1, const double* S2, int64_t n2, int64_t ld2, int32_t d, int32_t cov_mode,
                                 int32_t kmax, const double* w, const double* logl, const int64_t* prefix, int32_t nprefix, double* dotp,
                                 double* loglmax, double* jacobian, int32_t device)
{
    return feed_prefix_impl(false, S1, n1, ld1, S2, n2, ld2, d, cov_mode, kmax, w, logl, prefix, nprefix, dotp, loglmax, jacobian, device);
}

int mce_evidence_feed_prefix_dev_f64(const double* dS1, int64_t n1, int64_t ld1, const double* dS2, int64_t n2, int64_t ld2, int32_t d, int32_t cov_mode,
                                     int32_t kmax, const double* d_w, const double* d_logl, const int64_t* prefix, int32_t nprefix, double* dotp,
                                     double* loglmax, double* jacobian, int32_t device)
{
    return feed_prefix_impl(true, dS1, n1, ld1, dS2, n2, ld2, d, cov_mode, kmax, d_w, d_logl, prefix, nprefix, dotp, loglmax, jacobian, device);
}

}  // extern "C"
