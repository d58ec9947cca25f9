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
    int nsearch = 0, nsys = 0, nblk_max = 0, nblk_dotp = 0;
    size_t wsb = 0, vws = 0, dev_bytes = 0, host_bytes = 0;
    size_t o_S = 0, o_X = 0, o_W = 0, o_L = 0, o_F = 0, o_P = 0, o_lmax = 0, o_blk = 0, o_O = 0, o_small = 0, o_part = 0, o_ws = 0, o_vd = 0, o_vw = 0,
           o_vr = 0, o_dp = 0;
    char* dbase = nullptr;
    char* hbase = nullptr;
    bool dev_eig = false;               // the eigen-systems on the device: stage B is skipped
    size_t o_eig = 0;                   // its output, nsys slots each: evec | scale | lam | status

    double* e_evec(int i) const { return reinterpret_cast<double*>(dbase + o_eig) + (size_t)i * d * d; }
    double* e_scale(int i) const { return e_evec(nsys) + (size_t)i * d; }
    double* e_lam(int i) const { return e_scale(nsys) + (size_t)i * d; }
    int32_t* e_status(int i) const { return reinterpret_cast<int32_t*>(e_lam(nsys)) + i * mce_eig::kStatInts; }
    size_t e_back_bytes() const { return (size_t)nsys * (d * sizeof(double) + mce_eig::kStatInts * sizeof(int32_t)); }          // lam | status: one copy
    bool cross() const { return S2 != nullptr; }
    int64_t size_of(int i) const { return prefix[first[i]]; }
    double* dS1() const { return reinterpret_cast<double*>(dbase + o_S); }
    double* dS2() const { return dS1() + (size_t)n1 * d; }
    double* dX() const { return reinterpret_cast<double*>(dbase + o_X); }          // mode 1: the whitened prefix
    double* dW() const { return reinterpret_cast<double*>(dbase + o_W); }
    double* dL() const { return reinterpret_cast<double*>(dbase + o_L); }
    double* dF() const { return reinterpret_cast<double*>(dbase + o_F); }
    int64_t* dP() const { return reinterpret_cast<int64_t*>(dbase + o_P); }
    double* d_lmax() const { return reinterpret_cast<double*>(dbase + o_lmax); }
    double* d_blk() const { return reinterpret_cast<double*>(dbase + o_blk); }
    double* dO() const { return reinterpret_cast<double*>(dbase + o_O); }           // [B][kmax]
    double* d_mean3() const { return reinterpret_cast<double*>(dbase + o_small); }
    double* d_evec() const { return d_mean3() + 3 * 64; }
    double* d_scale() const { return d_evec() + (size_t)d * d; }
    double* d_cov(int i) const { return d_scale() + d + (size_t)i * d * d; }        // nsys slots, contiguous
    double* d_part() const { return reinterpret_cast<double*>(dbase + o_part); }
    char* ws() const { return dbase + o_ws; }
    double* d_vdist() const { return reinterpret_cast<double*>(dbase + o_vd); }
    int32_t* d_vres(int i) const { return reinterpret_cast<int32_t*>(dbase + o_vr) + 2 * i; }
    double* d_dpart() const { return reinterpret_cast<double*>(dbase + o_dp); }     // cross: [B][nblk_dotp][kmax]
    // pinned: cov / evec [nsys][d*d] (the eigenvectors replace the covariance they were solved from) | scale [nsys][d] |
    //         dotp [B][kmax] | lmax [B] | verify [nsearch][2]
    double* h_sys(int i) const { return reinterpret_cast<double*>(hbase) + (size_t)i * d * d; }
    double* h_scale(int i) const { return h_sys(nsys) + (size_t)i * d; }
    double* h_dotp() const { return h_scale(nsys); }
    double* h_lmax() const { return h_dotp() + (size_t)B * kmax; }
    int* h_verify(int i) const { return reinterpret_cast<int*>(h_lmax() + B) + 2 * i; }
    double* h_elam(int i) const { return h_lmax() + B + nsearch + 1 + (size_t)i * d; }          // device eigen-solver: lam [nsys][d] | status [nsys]
    int32_t* h_estatus(int i) const { return reinterpret_cast<int32_t*>(h_elam(nsys)) + i * mce_eig::kStatInts; }
};

// argument checks + sizes; no device work
int prefix_plan(PrefixJob& j, const double* dotp, const double* loglmax, const double* jacobian)
{
    if (!j.S1 || !j.w || !j.logl || !j.prefix || !dotp || !loglmax || !jacobian) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (j.B < 1 || j.B > MCE_MAX_PREFIX) return fail(MCE_ERR_INVALID, "nprefix=%d must lie in 1..%d", j.B, MCE_MAX_PREFIX);
    if (j.n1 < 2 || j.d < 1 || j.ld1 < j.d || (j.S2 && (j.n2 < 1 || j.ld2 < j.d)) || (j.cov_mode != 0 && j.cov_mode != 1))
        return fail(MCE_ERR_INVALID, "invalid sizes n1=%lld ld1=%lld n2=%lld ld2=%lld d=%d cov_mode=%d", (long long)j.n1, (long long)j.ld1,
                    (long long)j.n2, (long long)j.ld2, j.d, j.cov_mode);
    if (j.d > kFeedMaxDim) return fail(MCE_ERR_DIM_RANGE, "device feeders support d <= %d (got %d)", kFeedMaxDim, j.d);
    if (j.cov_mode == 1 && j.S2)
        return fail(MCE_ERR_INVALID, "cov_mode 1 with S2: the two sets' own eigen-systems depend on the solver's conventions; not offered for prefixes");
    j.k0 = j.S2 ? 0 : 1;
    j.K = j.kmax - j.k0;
    if (j.kmax <= j.k0) return fail(MCE_ERR_INVALID, "kmax=%d must exceed k0=%d", j.kmax, j.k0);
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
    int64_t vrows = 0;
    for (int i = 0; i < j.nsearch; ++i) {
        const int64_t nq = j.cross() ? j.pmax : j.size_of(i), nref = j.cross() ? j.n2 : nq;
        const int rc = make_plan(nq, nref, j.d, j.K, j.k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, j.plans[i]);
        if (rc != MCE_OK) return rc;
        j.wsb = std::max(j.wsb, j.plans[i].total + dotp_ws_bytes(nq, j.kmax));      // (plans need not grow with p: the maximum)
        if (j.d <= mce::kVerifyMaxDim && j.K <= mce::kVerifyMaxK) j.nverify[i] = (int)std::min<int64_t>(eff_verify(j.plans[i].filter(), nq), nq);
        if (j.nverify[i] > 0) {
            vrows = std::max(vrows, nq);
            j.vws = std::max(j.vws, mce_verify_workspace_bytes(j.nverify[i], j.K));
        }
    }
    if (j.cross()) vrows = j.pmax;          // the reductions read the search's distances
    const int d = j.d, npair = d * (d + 1) / 2;
    j.nblk_max = (int)((j.pmax + mce::kPrefixMaxRows - 1) / mce::kPrefixMaxRows);
    j.nblk_dotp = (int)((j.pmax + mce::kPrefixThreads - 1) / mce::kPrefixThreads);
    size_t off = 0;
    j.o_S = off;     off = align_up(off + (size_t)j.ntot * d * sizeof(double), 256);
    j.o_X = off;     off = align_up(off + (j.cov_mode == 1 ? (size_t)j.pmax * d * sizeof(double) : 0), 256);
    j.o_W = off;     off = align_up(off + (size_t)j.n1 * sizeof(double), 256);
    j.o_L = off;     off = align_up(off + (size_t)j.n1 * sizeof(double), 256);
    j.o_F = off;     off = align_up(off + (size_t)j.pmax * sizeof(double), 256);
    j.o_P = off;     off = align_up(off + (size_t)j.B * sizeof(int64_t), 256);
    j.o_lmax = off;  off = align_up(off + (size_t)j.B * sizeof(double), 256);
    j.o_blk = off;   off = align_up(off + (size_t)j.B * j.nblk_max * sizeof(double), 256);
    j.o_O = off;     off = align_up(off + (size_t)j.B * j.kmax * sizeof(double), 256);
    j.o_small = off; off = align_up(off + ((size_t)3 * 64 + (size_t)d * d + d + (size_t)j.nsys * d * d) * sizeof(double), 256);     // mean3 | evec | scale | cov slots
    j.o_part = off;  off = align_up(off + (size_t)std::max<int64_t>((int64_t)mce::kCovBlocks * npair, (int64_t)mce::kMeanBlocks * mce::kStatStride) * sizeof(double), 256);
    j.o_ws = off;    off = align_up(off + j.wsb, 256);
    j.o_vd = off;    off = align_up(off + (size_t)vrows * j.K * sizeof(double), 256);
    j.o_vw = off;    off = align_up(off + j.vws, 256);
    j.o_vr = off;    off = align_up(off + (size_t)j.nsearch * 2 * sizeof(int), 256);
    j.o_dp = off;    off = align_up(off + (j.cross() ? (size_t)j.B * j.nblk_dotp * j.kmax * sizeof(double) : 0), 256);
    j.dev_eig = eff_eig_mode() == 2;
    if (j.dev_eig) {
        j.o_eig = off;
        off = align_up(off + (size_t)j.nsys * (d * d + 2 * d) * sizeof(double) + (size_t)j.nsys * mce_eig::kStatInts * sizeof(int32_t), 256);
    }
    j.dev_bytes = off;
    j.host_bytes = align_up(((size_t)j.nsys * (d * d + d) + (size_t)j.B * j.kmax + j.B + j.nsearch + 1) * sizeof(double) + (j.dev_eig ? j.e_back_bytes() : 0), 64);
    return MCE_OK;
}

// upload, the B shifts, the covariance(s); everything enqueued on st, the small results on their way to the pinned arena
int prefix_stage_a(PrefixJob& j, hipStream_t st)
{
    const int d = j.d;
    const size_t row = (size_t)d * sizeof(double);
    const hipMemcpyKind kind = j.src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    MCE_HIP(hipMemcpy2DAsync(j.dS1(), row, j.S1, (size_t)j.ld1 * sizeof(double), row, (size_t)j.n1, kind, st));
    if (j.S2) MCE_HIP(hipMemcpy2DAsync(j.dS2(), row, j.S2, (size_t)j.ld2 * sizeof(double), row, (size_t)j.n2, kind, st));
    MCE_HIP(hipMemcpyAsync(j.dW(), j.w, (size_t)j.n1 * sizeof(double), kind, st));
    MCE_HIP(hipMemcpyAsync(j.dL(), j.logl, (size_t)j.n1 * sizeof(double), kind, st));
    MCE_HIP(hipMemcpyAsync(j.dP(), j.prefix, (size_t)j.B * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(mce::prefix_max_kernel, dim3((unsigned)j.nblk_max), dim3(mce::kPrefixThreads), 0, st, j.dL(), j.dP(), j.B, j.d_blk(), j.nblk_max);
    MCE_HIP(hipGetLastError());
    hipLaunchKernelGGL(mce::prefix_max_final_kernel, dim3(1), dim3(mce::kPrefixThreads), 0, st, j.d_blk(), j.dP(), j.B, j.nblk_max, j.d_lmax());
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(j.h_lmax(), j.d_lmax(), (size_t)j.B * sizeof(double), hipMemcpyDeviceToHost, st));
    // "all": ONE eigen-system from every row of s1 U s2, whatever the prefix (reference :1034-1037); "single": each prefix's own
    for (int i = 0; i < j.nsys; ++i) {
        const int rc = launch_covariance(j.dS1(), j.cov_mode == 0 ? j.ntot : j.size_of(i), d, j.d_part(), j.d_mean3(), j.d_cov(i), st);
        if (rc != MCE_OK) return rc;
    }
    if (j.dev_eig) return launch_eig(j.d_cov(0), d, j.nsys, j.e_evec(0), j.e_scale(0), j.e_lam(0), j.e_status(0), st);      // all systems, one launch
    MCE_HIP(hipMemcpyAsync(j.h_sys(0), j.d_cov(0), (size_t)j.nsys * d * d * sizeof(double), hipMemcpyDeviceToHost, st));
    return MCE_OK;
}

// the eigen-systems, on the host; jac[i] of system i
int prefix_stage_b(PrefixJob& j, std::vector<double>& jac)
{
    jac.assign(j.nsys, 0.0);
    for (int i = 0; i < j.nsys; ++i) {
        std::vector<double> lam;
        const int rc = feed_eig_system(j.h_sys(i), j.d, j.h_sys(i), j.h_scale(i), lam);
        if (rc != MCE_OK) {
            if (j.cov_mode == 0) return rc;
            const std::string msg = g_err;
            return fail(rc, "prefix %d (%lld rows): %s", j.first[i], (long long)j.size_of(i), msg.c_str());
        }
        g_eig_stats.host += 1;
        jac[i] = feed_jacobian(lam);
    }
    return MCE_OK;
}

int prefix_upload_system(PrefixJob& j, int i, hipStream_t st);

// the same from the device solver's results, once the call has finished: the first system that failed names the error
int prefix_eig_results(PrefixJob& j, std::vector<double>& jac)
{
    jac.assign(j.nsys, 0.0);
    for (int i = 0; i < j.nsys; ++i) eig_stats_add(g_eig_stats, j.h_estatus(i));
    for (int i = 0; i < j.nsys; ++i) {
        if (j.h_estatus(i)[mce_eig::kStatCode] != mce_eig::kStatusOk) {
            const int rc = eig_status_fail(j.h_estatus(i), j.h_elam(i));
            if (j.cov_mode == 0) return rc;
            const std::string msg = g_err;
            return fail(rc, "prefix %d (%lld rows): %s", j.first[i], (long long)j.size_of(i), msg.c_str());
        }
        jac[i] = feed_jacobian(std::vector<double>(j.h_elam(i), j.h_elam(i) + j.d));
    }
    return MCE_OK;
}

// the whitening of system i's rows: from the host's solve (uploaded here) or from the device solver's slot, with its status
int prefix_whiten(PrefixJob& j, int i, int64_t n, double* out, hipStream_t st)
{
    if (j.dev_eig) return launch_whiten(j.dS1(), n, j.d, j.e_evec(i), j.e_scale(i), out, st, j.e_status(i));
    const int rc = prefix_upload_system(j, i, st);
    return rc == MCE_OK ? launch_whiten(j.dS1(), n, j.d, j.d_evec(), j.d_scale(), out, st) : rc;
}

int prefix_upload_system(PrefixJob& j, int i, hipStream_t st)
{
    MCE_HIP(hipMemcpyAsync(j.d_evec(), j.h_sys(i), (size_t)j.d * j.d * sizeof(double), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(j.d_scale(), j.h_scale(i), (size_t)j.d * sizeof(double), hipMemcpyHostToDevice, st));
    return MCE_OK;
}

int prefix_fs(PrefixJob& j, int64_t p, int b, hipStream_t st)
{
    hipLaunchKernelGGL(mce::prefix_fs_kernel, dim3((unsigned)((p + mce::kPrefixThreads - 1) / mce::kPrefixThreads)), dim3(mce::kPrefixThreads), 0, st,
                       j.dL(), p, j.d_lmax() + b, j.dF());
    MCE_HIP(hipGetLastError());
    return MCE_OK;
}

// mce_options.verify, as in feed_stage_c: re-check a sample of the rows of search i (stream-ordered; the rows are still there)
int prefix_verify(PrefixJob& j, int i, const double* X, int64_t nq, const double* Y, int64_t nref, hipStream_t st)
{
    if (j.nverify[i] <= 0) return MCE_OK;
    const int rc = mce_verify_knn_f64_dev(X, nq, Y, nref, j.d, j.K, j.k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, 0, j.d_vdist(), j.K, j.nverify[i],
                                          0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1), j.d_vres(i), j.dbase + j.o_vw,
                                          mce_verify_workspace_bytes(j.nverify[i], j.K), st);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(j.h_verify(i), j.d_vres(i), 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    return MCE_OK;
}

// whitening, the searches and the reductions
int prefix_stage_c(PrefixJob& j, hipStream_t st)
{
    int rc = whiten_attr_once();
    if (rc != MCE_OK) return rc;
    const int d = j.d;
    if (j.cov_mode == 0) {
        rc = prefix_whiten(j, 0, j.ntot, j.dS1(), st);
        if (rc != MCE_OK) return rc;
    }
    SameSetHint hint(!j.cross());          // as in prefix_plan: the workspace was sized with it
    if (j.cross()) {
        // ONE search of the longest prefix against all of s2; its distances serve every batch
        rc = prefix_fs(j, j.pmax, j.B - 1, st);
        if (rc != MCE_OK) return rc;
        rc = mce_knn_dotp_f64_dev(j.dS1(), j.pmax, j.dS2(), j.n2, d, j.kmax, 0, 0, j.dW(), j.dF(), j.dO(), j.d_vdist(), j.ws(), j.wsb, st);
        if (rc != MCE_OK) return rc;
        hipLaunchKernelGGL(mce::prefix_dotp_kernel, dim3((unsigned)j.nblk_dotp, (unsigned)j.B), dim3(mce::kPrefixThreads), 0, st, j.d_vdist(), j.K, j.kmax, d,
                           ln_unit_ball(d), j.dW(), j.dL(), j.d_lmax(), j.dP(), j.d_dpart());
        MCE_HIP(hipGetLastError());
        hipLaunchKernelGGL(mce::prefix_dotp_final_kernel, dim3((unsigned)j.kmax, (unsigned)j.B), dim3(mce::kPrefixThreads), 0, st, j.d_dpart(),
                           (int64_t)j.nblk_dotp, j.kmax, j.dO());
        MCE_HIP(hipGetLastError());
        rc = prefix_verify(j, 0, j.dS1(), j.pmax, j.dS2(), j.n2, st);
        if (rc != MCE_OK) return rc;
    } else {
        for (int i = 0; i < j.nsearch; ++i) {
            const int b = j.first[i];
            const int64_t p = j.size_of(i);
            const double* X = j.dS1();
            if (j.cov_mode == 1) {          // the prefix's own system: out of place, the raw rows serve the next prefix
                rc = prefix_whiten(j, i, p, j.dX(), st);
                if (rc != MCE_OK) return rc;
                X = j.dX();
            }
            rc = prefix_fs(j, p, b, st);
            if (rc != MCE_OK) return rc;
            rc = mce_knn_dotp_f64_dev(X, p, X, p, d, j.kmax, 1, 0, j.dW(), j.dF(), j.dO() + (size_t)b * j.kmax, j.nverify[i] > 0 ? j.d_vdist() : nullptr,
                                      j.ws(), j.wsb, st);
            if (rc == MCE_OK) rc = prefix_verify(j, i, X, p, X, p, st);
            if (rc != MCE_OK) {
                const std::string msg = g_err;
                return fail(rc, "prefix %d (%lld rows): %s", b, (long long)p, msg.c_str());
            }
        }
    }
    MCE_HIP(hipMemcpyAsync(j.h_dotp(), j.dO(), (size_t)j.B * j.kmax * sizeof(double), hipMemcpyDeviceToHost, st));
    if (j.dev_eig) MCE_HIP(hipMemcpyAsync(j.h_elam(0), j.e_lam(0), j.e_back_bytes(), hipMemcpyDeviceToHost, st));
    return MCE_OK;
}

int prefix_stage_d(PrefixJob& j, const std::vector<double>& jac, double* dotp, double* loglmax, double* jacobian)
{
    for (int b = 0; b < j.B; ++b) {
        // equal prefixes were computed once: the first of them holds the sums (cross: every entry was reduced)
        const int src = j.cross() ? b : j.first[j.which[b]];
        std::copy(j.h_dotp() + (size_t)src * j.kmax, j.h_dotp() + (size_t)(src + 1) * j.kmax, dotp + (size_t)b * j.kmax);
        loglmax[b] = j.h_lmax()[b];
        jacobian[b] = jac[j.cov_mode == 1 ? j.which[b] : 0];
    }
    int checked = 0;
    for (int i = 0; i < j.nsearch; ++i) {
        if (j.nverify[i] <= 0) continue;
        checked += j.h_verify(i)[0];
        if (j.h_verify(i)[1] != 0) {
            g_last_verify_rows.store(checked);
            const int b = j.cross() ? j.B - 1 : j.first[i];
            return fail(MCE_ERR_VERIFY, "prefix %d (%lld rows): k-NN re-check failed: %d of %d sampled query rows have a neighbour list that an exact fp64 scan of "
                        "all %lld reference rows contradicts", b, (long long)j.prefix[b], j.h_verify(i)[1], j.h_verify(i)[0],
                        (long long)(j.cross() ? j.n2 : j.prefix[b]));
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
    // destroyed BEFORE the arena: an early return must not hand the arena back while kernels still run on it
    struct Quiesce {
        bool armed = true;
        ~Quiesce() { if (armed) (void)hipDeviceSynchronize(); }
    } quiesce;
    MCE_HIP(arena.alloc(j.dev_bytes));
    MCE_HIP(g_pinned.reserve(j.host_bytes));
    j.dbase = static_cast<char*>(arena.p);
    j.hbase = static_cast<char*>(g_pinned.p);
    hipStream_t st = nullptr;
    std::vector<double> jac;
    rc = prefix_stage_a(j, st);
    if (rc != MCE_OK) return rc;
    if (!j.dev_eig) {
        MCE_HIP(hipStreamSynchronize(st));
        rc = prefix_stage_b(j, jac);
        if (rc != MCE_OK) return rc;
    }
    rc = prefix_stage_c(j, st);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipStreamSynchronize(st));
    quiesce.armed = false;
    if (j.dev_eig) {          // the solves' status first: a failed system's searches ran on placeholder rows
        rc = prefix_eig_results(j, jac);
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
