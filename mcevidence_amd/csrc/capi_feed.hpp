// capi_feed.hpp -- part of capi.hip: the host-pointer fused call on one device, the evidence feed (covariance -> eigen-system ->
// whitening -> search -> reduction, MCEvidence.py:842-947 + :1093-1117) as a pipelined batch, and their entry points.  Where a job's
// arrays lie on the device and in the pinned block is feed_layout.hpp's; the stages that the convergence batches (capi_prefix.hpp)
// share with the feed -- the checks, the copy in, the host's solves, the device solver's results, the certificate -- are defined here.
#pragma once
#include "feed_layout.hpp"
namespace {

// (the host eigen-solver, jacobi_eig, lives in eig_jacobi.hpp with the rules it shares with the device solver)

// covariance (two-pass, unweighted, n-1) of the device matrix S[n, d] -> device cov[d*d]; enqueue only
int launch_covariance(const double* dS, int64_t n, int d, double* scratch_partial, double* d_mean3, double* d_cov, hipStream_t st)
{
    if (d > 63) {           // (the wide feeders, 64 <= d <= kFeedMaxDim: the means take 128 of the 192 doubles at d_mean3)
        hipLaunchKernelGGL(mce::col_mean_wide_partial_kernel, dim3(mce::kMeanBlocks), dim3(256), 0, st, dS, n, d, scratch_partial);
        MCE_HIP(hipGetLastError());
        hipLaunchKernelGGL(mce::col_mean_wide_final_kernel, dim3(1), dim3(128), 0, st, scratch_partial, n, d, d_mean3);
        MCE_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(mce::col_stats_partial_kernel, dim3(mce::kMeanBlocks), dim3(mce::kMeanThreads), 0, st, dS, n, d, scratch_partial);
        MCE_HIP(hipGetLastError());
        hipLaunchKernelGGL(mce::col_stats_final_kernel, dim3(1), dim3(64), 0, st, scratch_partial, n, d, d_mean3, (double*)nullptr);
        MCE_HIP(hipGetLastError());
    }
    for (int p0 = 0; p0 < d * (d + 1) / 2; p0 += mce::kCovPairsPerLaunch) {
        hipLaunchKernelGGL(mce::cov_partial_kernel, dim3(mce::kCovBlocks), dim3(mce::kCovThreads), (size_t)mce::kCovTileRows * d * sizeof(double), st,
                           dS, n, d, d_mean3, scratch_partial, p0);
        MCE_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(mce::cov_final_kernel, dim3(1), dim3(mce::kCovThreads), 0, st, scratch_partial, n, d, d_cov);
    MCE_HIP(hipGetLastError());
    return MCE_OK;
}
// the doubles of scratch_partial: the covariance kernels' partials or the mean kernels', whichever are more
size_t feed_part_doubles(int d)
{
    return (size_t)std::max<int64_t>((int64_t)mce::kCovBlocks * (d * (d + 1) / 2), (int64_t)mce::kMeanBlocks * mce::kStatStride);
}
static_assert(mce_feed::kMean3 == 3 * mce::kMaxDimPad, "the mean block of the covariance kernels");

// one device's share of the fused path: queries [q_lo, q_hi)
int fused_on_device(int device, const double* X, int64_t q_lo, int64_t q_hi, const double* Y, int64_t nr, int32_t d,
                    int32_t kmax, int32_t k0, int64_t self_offset, const double* w, const double* fs,
                    double* dotp_part, double* dist_out)
{
    const int64_t nq = q_hi - q_lo;
    const int K = kmax - k0;
    int rc = select_device(device);
    if (rc != MCE_OK) return rc;
    const double* Xs = X + q_lo * (int64_t)d;
    SameSetHint hint(Xs == Y && nq == nr && self_offset + q_lo == 0);
    Plan p;
    rc = make_plan(nq, nr, d, K, k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, p);
    if (rc != MCE_OK) return rc;
    const size_t wsb = p.total + dotp_ws_bytes(nq, kmax);
    DevBuf dX, dY, dW, dF, dO, dD, ws;
    const double* dXp = nullptr;
    rc = upload_rows(Xs, nq, Y, nr, d, dX, dY, dXp);
    if (rc != MCE_OK) return rc;
    MCE_HIP(dW.alloc((size_t)nq * sizeof(double)));
    MCE_HIP(dF.alloc((size_t)nq * sizeof(double)));
    MCE_HIP(dO.alloc((size_t)kmax * sizeof(double)));
    const int nverify = (d <= mce::kVerifyMaxDim && K <= mce::kVerifyMaxK) ? eff_verify(p.filter(), nq) : 0;     // mce_options.verify (default: on behind the fp16 filter)
    if (dist_out || nverify) MCE_HIP(dD.alloc((size_t)nq * K * sizeof(double)));
    MCE_HIP(ws.alloc(wsb));
    MCE_HIP(hipMemcpy(dW.p, w + q_lo, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dF.p, fs + q_lo, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    rc = mce_knn_dotp_f64_dev(dXp, nq, dY.as<double>(), nr, d, kmax, k0, self_offset + q_lo,
                              dW.as<double>(), dF.as<double>(), dO.as<double>(), (dist_out || nverify) ? dD.as<double>() : nullptr,
                              ws.p, wsb, nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipDeviceSynchronize());
    MCE_HIP(hipMemcpy(dotp_part, dO.p, (size_t)kmax * sizeof(double), hipMemcpyDeviceToHost));
    if (dist_out) MCE_HIP(hipMemcpy(dist_out + q_lo * (int64_t)K, dD.p, (size_t)nq * K * sizeof(double), hipMemcpyDeviceToHost));
    g_last_verify_rows.store(0);
    if (nverify)
        return verify_after_search(dXp, nq, dY.as<double>(), nr, d, K, k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, self_offset + q_lo, dD.as<double>(), K, nverify);
    return MCE_OK;
}

// `work(i)` (-> its code, its text in g_err) for each of the first n devices: on the caller's thread for one device, else one thread
// per device, the caller's options inherited (g_err is thread-local: each text is collected).  The first failing device is reported.
template <class Work> int for_each_device(const std::vector<int>& devs, int n, Work work)
{
    std::vector<int> rcs(n, MCE_OK);
    std::vector<std::string> errs(n);
    auto run = [&](int i) {
        rcs[i] = work(i);
        if (rcs[i] != MCE_OK) errs[i] = g_err;
    };
    if (n == 1) {
        run(0);
    } else {
        std::vector<std::thread> th;
        const CallOptions inherited = t_opt;
        for (int i = 0; i < n; ++i) th.emplace_back([&, i]() { t_opt = inherited; run(i); });
        for (auto& t : th) t.join();
    }
    for (int i = 0; i < n; ++i)
        if (rcs[i] != MCE_OK) return fail(rcs[i], "device %d: %s", devs[i], errs[i].c_str());
    return MCE_OK;
}
std::vector<int> device_list(const int32_t* devices, int32_t ndev) { return (!devices || ndev <= 0) ? std::vector<int>{0} : std::vector<int>(devices, devices + ndev); }

constexpr int kFeedMaxDim = 127;      // device feeders: d <= 63 on the narrow kernels, 64..127 on the wide ones (round 5; the search: knn_mfma.hpp's wide form)
static_assert(kFeedMaxDim <= mce::kWideMaxDim && mce::whiten_wide_lds_bytes(kFeedMaxDim) <= 160 * 1024, "wide feeders");
// ---- evidence feed: covariance -> eigen-system -> whitening -> search -> reduction ---------------
// One problem is four stages; only B runs on the host:
//   A  upload the raw rows, enqueue the covariance kernels, copy cov back (async, pinned)
//   B  d x d Jacobi eigen-solve, whitening scales, Jacobian
//   C  upload eVec/scale, whiten in place, fused search + reduction, copy dotp back (async, pinned)
//   D  hand the results to the caller
// With the device eigen-solver (mce_options.eig_mode 2, capi_eig.hpp) A ends with the solver's launch on the job's stream, B is
// skipped, C whitens from the solver's device-side output and copies the eigenvalues and the solve's status back behind the
// sums, and D reads the status first: a problem waits once, a batch once per wave (docs/design/device_eig.md).
// A batch is pipelined two deep in groups of kFeedGroup problems: while the device runs stage C of
// group g, the host performs the (blocking, pageable) uploads of group g+1 and that group's
// covariance kernels run beside the searches on a second stream set.  The searches themselves fill
// the device (make_plan splits the reference set of a small problem over all CUs), so the gain is
// hiding the PCIe upload, the host eigen-solves and the per-problem synchronisations.  Problems are
// processed in waves bounded by kWaveBytes of device memory.
constexpr size_t kWaveBytes = (size_t)8 << 30;
constexpr int kWaveMaxJobs = 1024;
constexpr int kFeedStreams = 4;   // per set (upload+covariance | whiten+search)
constexpr int kFeedGroup = 8;     // problems per pipeline step

// what a job is handed: the rows, the weights and the likelihood terms (the convergence batches: the log-likelihoods)
struct FeedIn { const double *S1, *S2, *w, *f; int64_t n1, ld1, n2, ld2; int d; };

struct FeedJob {
    mce_feed_problem* q = nullptr;
    int64_t index = 0;
    Plan plan;
    int k0 = 1, K = 0, rc = MCE_OK;
    int64_t nr = 0, ntot = 0;
    mce_feed::FeedSizes z;    // (nverify: a whole problem only, not a rank's share; dev_eig: mce_options.eig_mode 2, stage B is skipped)
    mce_feed::FeedArena a;    // this job's slice of the wave's device arena ...
    mce_feed::FeedPinned h;   // ... and of the pinned host arena
    double jac = 0.0;
    int part = 0, nparts = 1;         // one rank's share of the problem (mce_evidence_feed_part_f64); 1: all of it
    double* out_X = nullptr;          // mce_evidence_feed_whiten_f64: no search -- the whitened rows, the weights and the likelihood terms are left in
    double* out_w = nullptr;          // these DEVICE buffers of the caller's (auto evidence; the all-pairs-once partition searches them in several calls
    double* out_f = nullptr;          // with collectives in between: parallel.py)
    bool src_device = false;          // S1 / S2 / w / fs are DEVICE pointers (mce_evidence_feed_part_dev_f64: the node uploaded the chain once and
                                      // gathered it over xGMI): stage A copies device to device on the job's stream
    bool want_sum = false;            // fingerprint of the uploaded rows / weights / likelihoods (device-side)
    unsigned long long checksum = 0;
    int64_t q_lo = 0, q_hi = 0;       // cross evidence of a part: its rows of s1
    std::vector<double> lam;  // eigenvalues of the system that defines J (s1's in 'single' mode)
    EigStats eig;             // what this job solved where
    std::string err;
    hipEvent_t upload_ev = nullptr;   // orders the job's stream behind its blocking uploads
    ~FeedJob() { if (upload_ev) (void)hipEventDestroy(upload_ev); }
    FeedJob() = default;
    FeedJob(const FeedJob&) = delete;
    FeedJob& operator=(const FeedJob&) = delete;

    int d() const { return q->d; }
    FeedIn in() const { return FeedIn{q->S1, q->S2, q->w, q->fs, q->n1, q->ld1, q->n2, q->ld2, q->d}; }
    bool two_systems() const { return q->cov_mode == 1 && q->S2 != nullptr; }
    void place(void* dbase, void* hbase) { a = mce_feed::FeedArena(z, dbase), h = mce_feed::FeedPinned(z, hbase); }          // (null, null): the sizes only
    void set_error(int code) { rc = code; err = g_err; }
};

// the checks behind an entry point's own null-pointer check, in this order: the sizes, d, (the convergence batches: no two systems),
// kmax -- cross evidence counts from the nearest row (k0 = 0), auto evidence past the row itself (k0 = 1)
int feed_check(const FeedIn& in, int cov_mode, int kmax, bool one_system_only, int& k0, int& K)
{
    if (in.n1 < 2 || in.d < 1 || in.ld1 < in.d || (in.S2 && (in.n2 < 1 || in.ld2 < in.d)) || (cov_mode != 0 && cov_mode != 1))
        return fail(MCE_ERR_INVALID, "invalid sizes n1=%lld ld1=%lld n2=%lld ld2=%lld d=%d cov_mode=%d", (long long)in.n1, (long long)in.ld1,
                    (long long)in.n2, (long long)in.ld2, in.d, cov_mode);
    if (in.d > kFeedMaxDim) return fail(MCE_ERR_DIM_RANGE, "device feeders support d <= %d (got %d)", kFeedMaxDim, in.d);
    if (one_system_only && cov_mode == 1 && in.S2)
        return fail(MCE_ERR_INVALID, "cov_mode 1 with S2: the two sets' own eigen-systems depend on the solver's conventions; not offered for prefixes");
    k0 = in.S2 ? 0 : 1;
    K = kmax - k0;
    if (kmax <= k0) return fail(MCE_ERR_INVALID, "kmax=%d must exceed k0=%d", kmax, k0);
    return MCE_OK;
}

// the rows (packed to d columns), weights and likelihoods into the arena.  ev null: the copies on st.  Otherwise blocking copies, and
// *ev (created on first use), recorded behind them, orders st after them: see feed_stage_a.
int feed_copy_in(const FeedIn& in, double* dS1, double* dS2, double* dW, double* dF, hipMemcpyKind kind, hipStream_t st, hipEvent_t* ev)
{
    const size_t D = sizeof(double), row = (size_t)in.d * D, vec = (size_t)in.n1 * D;
    if (!ev) {
        MCE_HIP(hipMemcpy2DAsync(dS1, row, in.S1, (size_t)in.ld1 * D, row, (size_t)in.n1, kind, st));
        if (in.S2) MCE_HIP(hipMemcpy2DAsync(dS2, row, in.S2, (size_t)in.ld2 * D, row, (size_t)in.n2, kind, st));
        MCE_HIP(hipMemcpyAsync(dW, in.w, vec, kind, st));
        MCE_HIP(hipMemcpyAsync(dF, in.f, vec, kind, st));
        return MCE_OK;
    }
    MCE_HIP(hipMemcpy2D(dS1, row, in.S1, (size_t)in.ld1 * D, row, (size_t)in.n1, kind));
    if (in.S2) MCE_HIP(hipMemcpy2D(dS2, row, in.S2, (size_t)in.ld2 * D, row, (size_t)in.n2, kind));
    MCE_HIP(hipMemcpy(dW, in.w, vec, kind));
    MCE_HIP(hipMemcpy(dF, in.f, vec, kind));
    if (!*ev) MCE_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    MCE_HIP(hipEventRecord(*ev, nullptr));
    MCE_HIP(hipStreamWaitEvent(st, *ev, 0));
    return MCE_OK;
}

// destroyed BEFORE the arena it guards: an early return (a failing HIP call) must not hand the arena back to the pool while
// kernels -- of other jobs, on other streams -- are still running on it
struct Quiesce {
    bool armed = true;
    ~Quiesce() { if (armed) (void)hipDeviceSynchronize(); }
};

// argument checks + sizes; no device work
int feed_plan(FeedJob& j)
{
    const mce_feed_problem& q = *j.q;
    if (!q.S1 || !q.w || !q.fs || !q.dotp) return fail(MCE_ERR_INVALID, "null pointer argument");
    int rc = feed_check(j.in(), q.cov_mode, q.kmax, false, j.k0, j.K);
    if (rc != MCE_OK) return rc;
    j.nr = q.S2 ? q.n2 : q.n1;
    j.ntot = q.n1 + (q.S2 ? q.n2 : 0);
    SameSetHint hint(q.S2 == nullptr);          // auto evidence: one set; cross evidence: never the symmetric sweep
    rc = make_plan(q.n1, j.nr, q.d, j.K, j.k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, j.plan);
    if (rc != MCE_OK) return rc;
    mce_feed::FeedSizes& z = j.z;
    z.search_ws_bytes = j.out_X ? 0 : j.plan.total + dotp_ws_bytes(q.n1, q.kmax);
    j.q_lo = 0;
    j.q_hi = q.n1;
    if (j.nparts > 1 && q.S2) {
        // a part of a cross-evidence problem: contiguous rows of s1 against all of s2
        j.q_lo = q.n1 * j.part / j.nparts;
        j.q_hi = q.n1 * (int64_t)(j.part + 1) / j.nparts;
        if (j.q_hi > j.q_lo) {
            Plan shard;
            rc = make_plan(j.q_hi - j.q_lo, j.nr, q.d, j.K, MCE_SELF_NONE, shard);
            if (rc != MCE_OK) return rc;
            z.search_ws_bytes = std::max(z.search_ws_bytes, shard.total + dotp_ws_bytes(j.q_hi - j.q_lo, q.kmax));
        }
    }
    z.n1 = q.n1; z.ntot = j.ntot; z.d = q.d; z.kmax = q.kmax; z.K = j.K;
    z.nsys = j.two_systems() ? 2 : 1;
    z.part_doubles = feed_part_doubles(q.d);
    z.nverify = (j.nparts == 1 && !j.out_X && q.d <= mce::kVerifyMaxDim && j.K <= mce::kVerifyMaxK) ? (int)std::min<int64_t>(eff_verify(j.plan.filter(), q.n1), q.n1) : 0;
    z.verify_ws_bytes = mce_verify_workspace_bytes(z.nverify, j.K);
    z.dev_eig = eff_eig_mode() == 2;
    z.stat_ints = mce_eig::kStatInts;
    j.place(nullptr, nullptr);
    return MCE_OK;
}

int feed_stage_a(FeedJob& j, hipStream_t st)
{
    const mce_feed_problem& q = *j.q;
    const mce_feed::FeedArena& a = j.a;
    const int d = q.d;
    // Uploads: blocking copies from the caller's pageable arrays (measured faster than hipMemcpyAsync on the job's
    // non-blocking stream: 300 Planck-sized chains 0.131 vs 0.153 s), followed by an EXPLICIT dependency -- an event
    // recorded on the stream the copies ran on, waited for by the job's stream -- so the covariance kernels behind them
    // are ordered after the uploads by the API's rules, not by how this runtime happens to implement a pageable copy
    // (a blocking hipMemcpy from pageable memory only promises that the SOURCE has been consumed on return, and
    // hipStreamNonBlocking streams do not synchronise with the legacy default stream).  MCE_FEED_UPLOAD=async: the
    // copies themselves on the job's stream.  Rows that are on this device already (the caller has synchronised the
    // stream that produced them) are copied on the job's stream.
    const bool on_stream = j.src_device || env_feed_upload_async() || st == nullptr;
    int rc = feed_copy_in(j.in(), a.S1, a.S2, a.W, a.F, j.src_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st, on_stream ? nullptr : &j.upload_ev);
    if (rc != MCE_OK) return rc;
    if (j.want_sum) {
        // fingerprint of what this rank was handed (RAW rows, weights, fs), before anything is whitened in place
        MCE_HIP(mce::zero_async(a.sum, sizeof(unsigned long long), st));
        const int64_t nw[3] = {j.ntot * (int64_t)d, q.n1, q.n1};
        const double* src[3] = {a.S1, a.W, a.F};
        for (int b = 0; b < 3; ++b) {
            const unsigned blocks = (unsigned)std::min<int64_t>((nw[b] + mce::kSumThreads - 1) / mce::kSumThreads, 2048);
            hipLaunchKernelGGL(mce::checksum_kernel, dim3(blocks), dim3(mce::kSumThreads), 0, st, reinterpret_cast<const unsigned long long*>(src[b]), nw[b],
                               (unsigned long long)(b + 1) << 56 ^ (unsigned long long)q.n1 << 8 ^ (unsigned long long)d, a.sum);
            MCE_HIP(hipGetLastError());
        }
        MCE_HIP(hipMemcpyAsync(j.h.sum, a.sum, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    // "all": one eigen-system from s1 U s2; "single": s1's own, and s2's own for s2 (J stays s1's)
    const int64_t n_first = q.cov_mode == 0 ? j.ntot : q.n1;
    if (j.z.dev_eig) {
        // the covariances into the solver's slots, both systems of a 'single' cross evidence in ONE launch; nothing comes down
        rc = launch_covariance(a.S1, n_first, d, a.part, a.mean3, a.eig.cov_at(0), st);
        if (rc == MCE_OK && j.two_systems()) rc = launch_covariance(a.S2, q.n2, d, a.part, a.mean3, a.eig.cov_at(1), st);
        if (rc != MCE_OK) return rc;
        return launch_eig(a.eig.cov, d, j.z.nsys, a.eig.evec, a.eig.scale, a.eig.back.lam, a.eig.back.status, st);
    }
    rc = launch_covariance(a.S1, n_first, d, a.part, a.mean3, a.cov, st);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(j.h.cov_at(0), a.cov, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, st));
    if (j.two_systems()) {
        rc = launch_covariance(a.S2, q.n2, d, a.part, a.mean3, a.cov, st);
        if (rc != MCE_OK) return rc;
        MCE_HIP(hipMemcpyAsync(j.h.cov_at(1), a.cov, (size_t)d * d * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    return MCE_OK;
}

// one eigen-system of the feed (stage B): cov[d*d] (row-major, as the covariance kernels left it) -> evec[d*d], the whitening
// scales 1 / sqrt(lambda) and the eigenvalues (descending).  A covariance that is not finite or not positive definite fails.
int feed_eig_system(const double* h_cov, int d, double* evec, double* scale, std::vector<double>& lam)
{
    std::vector<double> cov(h_cov, h_cov + (size_t)d * d), V;
    jacobi_eig(cov, d, lam, V);
    for (int i = 0; i < d; ++i) {
        if (lam[i] != lam[i] || std::isinf(lam[i])) return fail(MCE_ERR_INVALID, "samples contain NaN or infinity (non-finite covariance)");
        if (!(lam[i] > 0.0)) return fail(MCE_ERR_INVALID, "math domain error: covariance eigenvalue %d is %g (use fewer parameters, ndim)", i, lam[i]);
    }
    std::copy(V.begin(), V.end(), evec);
    for (int i = 0; i < d; ++i) scale[i] = 1.0 / std::sqrt(lam[i]);
    return MCE_OK;
}

// J = sqrt(det cov) from the eigenvalues
double feed_jacobian(const std::vector<double>& lam)
{
    double logdet = 0.0;
    for (double x : lam) logdet += std::log(x);
    return std::exp(0.5 * logdet);
}

// the host's solves (stage B): system i from cov[i] into evec[i] (the same block will do) and scale[i], its eigenvalues into lam[i];
// counted into `stats`.  The first system that fails ends the loop: `at` is its index.
int feed_solve_host(int nsys, int d, const double* cov, double* evec, double* scale, std::vector<std::vector<double>>& lam, EigStats& stats, int& at)
{
    lam.assign(nsys, std::vector<double>());
    for (at = 0; at < nsys; ++at) {
        const int rc = feed_eig_system(cov + (size_t)at * d * d, d, evec + (size_t)at * d * d, scale + (size_t)at * d, lam[at]);
        if (rc != MCE_OK) return rc;
        stats.host += 1;
    }
    return MCE_OK;
}

// the same from the device solver, once its status words and eigenvalues are on the host: every system is counted into `stats`; the
// first that failed names the error (`at`: its index) -- its searches ran on placeholder rows, whatever their certificate says
int feed_eig_results(const mce_feed::EigBack& h, int nsys, EigStats& stats, int& at)
{
    for (int i = 0; i < nsys; ++i) eig_stats_add(stats, h.status_at(i));
    for (at = 0; at < nsys; ++at)
        if (h.status_at(at)[mce_eig::kStatCode] != mce_eig::kStatusOk) return eig_status_fail(h.status_at(at), h.lam_at(at));
    return MCE_OK;
}

int feed_stage_b(FeedJob& j)
{
    std::vector<std::vector<double>> lam;
    int at = 0;
    const int rc = feed_solve_host(j.z.nsys, j.d(), j.h.cov, j.h.evec, j.h.scale, lam, j.eig, at);
    if (rc != MCE_OK) return rc;
    j.lam = lam[0];
    j.jac = feed_jacobian(j.lam);
    return MCE_OK;
}

// out[r] = (S[r] . evec) * scale for the n rows of S (out may be S); evec / scale on the device already; enqueue only
// d_status (may be null): the device eigen-solve's status word; not 0 -> placeholder rows (feeders.hpp)
int launch_whiten(const double* S, int64_t n, int d, const double* d_evec, const double* d_scale, double* out, hipStream_t st, const int32_t* d_status = nullptr)
{
    if (d > 63)
        hipLaunchKernelGGL(mce::whiten_wide_kernel, dim3((unsigned)((n + mce::kWhitenRows - 1) / mce::kWhitenRows)), dim3(mce::kWhitenRows),
                           mce::whiten_wide_lds_bytes(d), st, S, n, d, d_evec, d_scale, out, d_status);
    else
        hipLaunchKernelGGL(mce::whiten_kernel, dim3((unsigned)((n + mce::kWhitenRows - 1) / mce::kWhitenRows)), dim3(mce::kWhitenRows),
                           mce::whiten_lds_bytes(d), st, S, n, d, d_evec, d_scale, out, d_status);
    MCE_HIP(hipGetLastError());
    return MCE_OK;
}

int feed_whiten(FeedJob& j, int sidx, double* rows, int64_t n, hipStream_t st)
{
    const int d = j.d();
    if (j.z.dev_eig) return launch_whiten(rows, n, d, j.a.eig.evec_at(sidx), j.a.eig.scale_at(sidx), rows, st, j.a.eig.back.status_at(sidx));
    MCE_HIP(hipMemcpyAsync(j.a.evec, j.h.evec_at(sidx), (size_t)d * d * sizeof(double), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(j.a.scale, j.h.scale_at(sidx), (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    return launch_whiten(rows, n, d, j.a.evec, j.a.scale, rows, st);
}

// the whitening kernels stage more LDS than the default limit: raise it once per device
int whiten_attr_once()
{
    static std::atomic<bool> attr_set[kMaxDevices];
    int dev = 0;
    MCE_HIP(hipGetDevice(&dev));
    if (dev < kMaxDevices && !attr_set[dev].load()) {
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::whiten_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)mce::whiten_lds_bytes(63)));
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::whiten_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mce::whiten_wide_lds_bytes(kFeedMaxDim)));
        attr_set[dev].store(true);
    }
    return MCE_OK;
}

// mce_options.verify: the rows a search ran on and its distances are still on the device; re-check a sample of nverify of them
// (stream-ordered; the call's search `index` seeds the sample) and send {rows checked, rows failed} to h_res
int feed_verify_enqueue(const double* X, int64_t nq, const double* Y, int64_t nref, int d, int K, int k0, const double* d_dist, int nverify, int64_t index,
                        int32_t* d_res, void* vws, int* h_res, hipStream_t st)
{
    const int rc = mce_verify_knn_f64_dev(X, nq, Y, nref, d, K, k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, 0, d_dist, K, nverify,
                                          0x9E3779B97F4A7C15ull * (unsigned long long)(index + 1), d_res, vws, mce_verify_workspace_bytes(nverify, K), st);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(h_res, d_res, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    return MCE_OK;
}

int feed_stage_c(FeedJob& j, hipStream_t st)
{
    const mce_feed_problem& q = *j.q;
    const mce_feed::FeedArena& a = j.a;
    const size_t wsb = j.z.search_ws_bytes;
    int rc = whiten_attr_once();
    if (rc != MCE_OK) return rc;
    if (j.two_systems()) {
        rc = feed_whiten(j, 0, a.S1, q.n1, st);
        if (rc != MCE_OK) return rc;
        rc = feed_whiten(j, 1, a.S2, q.n2, st);
    } else {
        rc = feed_whiten(j, 0, a.S1, q.cov_mode == 0 ? j.ntot : q.n1, st);
    }
    if (rc != MCE_OK) return rc;
    SameSetHint hint(q.S2 == nullptr);          // as in feed_plan: the workspace was sized with it
    if (j.out_X) {                              // whitening only: hand the rows over, no search (the sums stay zero)
        MCE_HIP(hipMemcpyAsync(j.out_X, a.S1, (size_t)q.n1 * q.d * sizeof(double), hipMemcpyDeviceToDevice, st));
        MCE_HIP(hipMemcpyAsync(j.out_w, a.W, (size_t)q.n1 * sizeof(double), hipMemcpyDeviceToDevice, st));
        MCE_HIP(hipMemcpyAsync(j.out_f, a.F, (size_t)q.n1 * sizeof(double), hipMemcpyDeviceToDevice, st));
        rc = (mce::zero_async(a.O, (size_t)q.kmax * sizeof(double), st) == hipSuccess) ? MCE_OK : fail(MCE_ERR_HIP, "clearing the sums failed");
    } else if (j.nparts > 1 && !q.S2)           // one rank's share of an auto-evidence search: the library's partition
        rc = mce_knn_dotp_part_f64_dev(a.S1, q.n1, q.d, q.kmax, j.part, j.nparts, a.W, a.F, a.O, a.ws, wsb, st);
    else if (j.nparts > 1 && j.q_hi <= j.q_lo)
        rc = (mce::zero_async(a.O, (size_t)q.kmax * sizeof(double), st) == hipSuccess) ? MCE_OK : fail(MCE_ERR_HIP, "clearing the sums failed");
    else if (j.nparts > 1)                      // ... of a cross-evidence search: its rows of s1 against all of s2
        rc = mce_knn_dotp_f64_dev(a.S1 + j.q_lo * (int64_t)q.d, j.q_hi - j.q_lo, a.S2, j.nr, q.d, q.kmax, 0, 0, a.W + j.q_lo, a.F + j.q_lo,
                                  a.O, nullptr, a.ws, wsb, st);
    else
        rc = mce_knn_dotp_f64_dev(a.S1, q.n1, q.S2 ? a.S2 : a.S1, j.nr, q.d, q.kmax, j.k0, 0, a.W, a.F, a.O, a.vdist, a.ws, wsb, st);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(j.h.dotp, a.O, (size_t)q.kmax * sizeof(double), hipMemcpyDeviceToHost, st));
    if (j.z.dev_eig) MCE_HIP(hipMemcpyAsync(j.h.eig.lam, a.eig.back.lam, a.eig.back.bytes, hipMemcpyDeviceToHost, st));
    if (j.z.nverify > 0)          // (a.vdist is there exactly then)
        return feed_verify_enqueue(a.S1, q.n1, q.S2 ? a.S2 : a.S1, j.nr, q.d, j.K, j.k0, a.vdist, j.z.nverify, j.index, a.vres, a.vws, j.h.verify, st);
    return MCE_OK;
}

void feed_stage_d(FeedJob& j)
{
    mce_feed_problem& q = *j.q;
    if (j.z.dev_eig) {
        int at = 0;
        const int rc = feed_eig_results(j.h.eig, j.z.nsys, j.eig, at);
        if (rc != MCE_OK) {
            j.set_error(rc);
            g_last_verify_rows.store(0);
            return;
        }
        j.lam.assign(j.h.eig.lam, j.h.eig.lam + q.d);
        j.jac = feed_jacobian(j.lam);
    }
    std::copy(j.h.dotp, j.h.dotp + q.kmax, q.dotp);
    q.jacobian = j.jac;
    if (q.eigenvalues) std::copy(j.lam.begin(), j.lam.end(), q.eigenvalues);
    if (j.want_sum) j.checksum = *j.h.sum;
    g_last_verify_rows.store(j.z.nverify > 0 ? j.h.verify[0] : 0);
    if (j.z.nverify > 0 && j.h.verify[1] != 0)
        j.set_error(fail(MCE_ERR_VERIFY, "k-NN re-check failed: %d of %d sampled query rows have a neighbour list that an exact fp64 scan of all %lld reference rows "
                         "contradicts", j.h.verify[1], j.h.verify[0], (long long)j.nr));
}

// all jobs of one device, in waves; per-job failures are recorded in the job, a failure of the
// machinery itself (allocation, stream) is returned
int feed_run_on_device(int device, std::vector<FeedJob*>& jobs)
{
    int rc = select_device(device);
    if (rc != MCE_OK) return rc;
    // two stream sets so that the covariance of the NEXT group never queues behind the searches of
    // the current one; a single problem runs on the default stream
    std::vector<hipStream_t> sa, sc;
    std::vector<hipEvent_t> events;
    struct Guard {
        std::vector<hipStream_t>&a, &c;
        std::vector<hipEvent_t>& e;
        ~Guard()
        {
            for (hipStream_t x : a) (void)hipStreamDestroy(x);
            for (hipStream_t x : c) (void)hipStreamDestroy(x);
            for (hipEvent_t x : e) (void)hipEventDestroy(x);
        }
    } guard{sa, sc, events};
    const bool piped = jobs.size() > 1;
    if (piped) {
        const int ns = (int)std::min<size_t>(kFeedStreams, jobs.size());
        for (int i = 0; i < ns; ++i) {
            hipStream_t s;
            MCE_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            sa.push_back(s);
            MCE_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            sc.push_back(s);
        }
        for (int i = 0; i < kFeedGroup; ++i) {
            hipEvent_t e;
            MCE_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            events.push_back(e);
        }
    }
    size_t wave_bytes = kWaveBytes;
    if (const size_t wb = read_tuning().feed_wave_bytes) wave_bytes = wb;   // tests: force several waves
    size_t lo = 0;
    while (lo < jobs.size()) {
        size_t hi = lo, dev_bytes = 0, host_bytes = 0;
        while (hi < jobs.size() && (hi == lo || (dev_bytes + jobs[hi]->a.total <= wave_bytes && hi - lo < (size_t)kWaveMaxJobs))) {
            dev_bytes += jobs[hi]->a.total;
            host_bytes += jobs[hi]->h.total;
            ++hi;
        }
        DevBuf arena;
        Quiesce quiesce;
        PinnedArena& pinned = g_pinned;
        MCE_HIP(arena.alloc(dev_bytes));
        MCE_HIP(pinned.reserve(host_bytes));
        size_t doff = 0, hoff = 0;
        for (size_t i = lo; i < hi; ++i) {
            jobs[i]->place(static_cast<char*>(arena.p) + doff, static_cast<char*>(pinned.p) + hoff);
            doff += jobs[i]->a.total;
            hoff += jobs[i]->h.total;
        }
        if (!piped) {
            FeedJob& j = *jobs[lo];
            if (j.rc == MCE_OK) {
                int r = feed_stage_a(j, nullptr);
                if (r == MCE_OK && !j.z.dev_eig) { MCE_HIP(hipStreamSynchronize(nullptr)); r = feed_stage_b(j); }
                if (r == MCE_OK) r = feed_stage_c(j, nullptr);
                if (r == MCE_OK) { MCE_HIP(hipStreamSynchronize(nullptr)); feed_stage_d(j); }
                else { j.set_error(r); (void)hipStreamSynchronize(nullptr); }
            }
            quiesce.armed = false;
            lo = hi;
            continue;
        }
        // groups of kFeedGroup problems, two deep: while the device searches group g the host uploads
        // group g+1 (blocking pageable copies) and its covariance kernels run beside the searches
        auto stage_a_group = [&](size_t g0, size_t g1) -> int {
            for (size_t i = g0; i < g1; ++i) {
                FeedJob& j = *jobs[i];
                if (j.rc != MCE_OK) continue;
                hipStream_t st = sa[i % sa.size()];
                const int r = feed_stage_a(j, st);
                if (r != MCE_OK) { j.set_error(r); continue; }
                MCE_HIP(hipEventRecord(events[i - g0], st));
            }
            return MCE_OK;
        };
        rc = stage_a_group(lo, std::min(hi, lo + (size_t)kFeedGroup));
        if (rc != MCE_OK) return rc;
        for (size_t g0 = lo; g0 < hi; g0 += kFeedGroup) {
            const size_t g1 = std::min(hi, g0 + (size_t)kFeedGroup);
            for (size_t i = g0; i < g1; ++i) {
                FeedJob& j = *jobs[i];
                if (j.rc != MCE_OK) continue;
                int r = MCE_OK;
                if (j.z.dev_eig) MCE_HIP(hipStreamWaitEvent(sc[i % sc.size()], events[i - g0], 0));      // the device waits for stage A, the host does not
                else { MCE_HIP(hipEventSynchronize(events[i - g0])); r = feed_stage_b(j); }
                if (r == MCE_OK) r = feed_stage_c(j, sc[i % sc.size()]);
                if (r != MCE_OK) j.set_error(r);
            }
            if (g1 < hi) {
                rc = stage_a_group(g1, std::min(hi, g1 + (size_t)kFeedGroup));
                if (rc != MCE_OK) return rc;
            }
        }
        for (hipStream_t st : sc) MCE_HIP(hipStreamSynchronize(st));
        for (hipStream_t st : sa) MCE_HIP(hipStreamSynchronize(st));     // (jobs that failed after stage A left work there)
        quiesce.armed = false;
        for (size_t i = lo; i < hi; ++i)
            if (jobs[i]->rc == MCE_OK) feed_stage_d(*jobs[i]);
        lo = hi;
    }
    return MCE_OK;
}

mce_feed_problem feed_problem(const double* S1, int64_t n1, int64_t ld1, const double* S2, int64_t n2, int64_t ld2, int32_t d, int32_t cov_mode, int32_t kmax,
                              const double* w, const double* fs, double* dotp, double* eigenvalues)
{
    mce_feed_problem q;
    std::memset(&q, 0, sizeof(q));
    q.S1 = S1; q.n1 = n1; q.ld1 = ld1;
    q.S2 = S2; q.n2 = S2 ? n2 : 0; q.ld2 = S2 ? ld2 : 0;
    q.d = d; q.cov_mode = cov_mode; q.kmax = kmax;
    q.w = w; q.fs = fs; q.dotp = dotp; q.eigenvalues = eigenvalues;
    return q;
}

// one job that is not a batch's (a rank's part, the whitening alone): `job` carries what makes it so; q.dotp takes the sums
int feed_run_one(FeedJob& job, mce_feed_problem& q, bool src_device, double* jacobian, uint64_t* checksum, int32_t device)
{
    job.q = &q;
    job.src_device = src_device;
    job.want_sum = checksum != nullptr;
    g_eig_stats = EigStats();
    int rc = feed_plan(job);
    if (rc != MCE_OK) return rc;
    std::vector<FeedJob*> jobs{&job};
    rc = feed_run_on_device(device, jobs);
    g_eig_stats = job.eig;
    if (rc != MCE_OK) return rc;
    if (job.rc != MCE_OK) return fail(job.rc, "%s", job.err.c_str());
    *jacobian = q.jacobian;
    if (checksum) *checksum = job.checksum;
    return MCE_OK;
}

}  // namespace

extern "C" {

size_t mce_feed_problem_size(void) { return sizeof(mce_feed_problem); }

static int feed_batch_impl(bool src_device, mce_feed_problem* problems, int64_t nprob, const int32_t* devices, int32_t ndev)
{
    if (nprob < 0 || (nprob > 0 && !problems)) return fail(MCE_ERR_INVALID, "invalid problem list");
    g_eig_stats = EigStats();
    if (nprob == 0) return MCE_OK;
    std::vector<FeedJob> jobs((size_t)nprob);
    for (int64_t i = 0; i < nprob; ++i) {
        jobs[i].q = &problems[i];
        jobs[i].index = i;
        jobs[i].src_device = src_device;
        problems[i].status = MCE_OK;
        problems[i].jacobian = 0.0;
        const int r = feed_plan(jobs[i]);
        if (r != MCE_OK) jobs[i].set_error(r);
    }
    const std::vector<int> devs = device_list(devices, ndev);
    const int n = (int)std::min<int64_t>((int64_t)devs.size(), nprob);
    // greedy balance by pair count (largest first), then restore the caller's order per device
    std::vector<std::vector<FeedJob*>> per_dev(n);
    if (n == 1) {
        for (auto& j : jobs) if (j.rc == MCE_OK) per_dev[0].push_back(&j);
    } else {
        std::vector<FeedJob*> order;
        for (auto& j : jobs) if (j.rc == MCE_OK) order.push_back(&j);
        std::stable_sort(order.begin(), order.end(), [](const FeedJob* a, const FeedJob* b) {
            return (double)a->q->n1 * (double)a->nr > (double)b->q->n1 * (double)b->nr;
        });
        std::vector<double> load(n, 0.0);
        for (FeedJob* j : order) {
            const int t = (int)(std::min_element(load.begin(), load.end()) - load.begin());
            load[t] += (double)j->q->n1 * (double)j->nr + 1e6;
            per_dev[t].push_back(j);
        }
        for (auto& v : per_dev) std::sort(v.begin(), v.end(), [](const FeedJob* a, const FeedJob* b) { return a->index < b->index; });
    }
    const int rc = for_each_device(devs, n, [&](int i) { return per_dev[i].empty() ? MCE_OK : feed_run_on_device(devs[i], per_dev[i]); });
    for (const FeedJob& j : jobs) eig_stats_merge(g_eig_stats, j.eig);
    if (rc != MCE_OK) return rc;
    int first = MCE_OK;
    for (int64_t i = 0; i < nprob; ++i) {
        problems[i].status = jobs[i].rc;
        if (jobs[i].rc != MCE_OK && first == MCE_OK) {
            first = jobs[i].rc;
            if (nprob == 1) fail(first, "%s", jobs[i].err.c_str());
            else fail(first, "problem %lld: %s", (long long)i, jobs[i].err.c_str());
        }
    }
    return first;
}

int mce_evidence_feed_batch_f64(mce_feed_problem* problems, int64_t nprob, const int32_t* devices, int32_t ndev)
{
    return feed_batch_impl(false, problems, nprob, devices, ndev);
}

int mce_evidence_feed_batch_dev_f64(mce_feed_problem* problems, int64_t nprob, int32_t device)
{
    if (device < 0) return fail(MCE_ERR_INVALID, "device %d", device);
    return feed_batch_impl(true, problems, nprob, &device, 1);
}

int mce_evidence_feed_f64(const double* S1, int64_t n1, int64_t ld1, const double* S2, int64_t n2, int64_t ld2,
                          int32_t d, int32_t cov_mode, int32_t kmax, const double* w, const double* fs,
                          double* dotp, double* jacobian, double* eigenvalues, int32_t device)
{
    if (!jacobian) return fail(MCE_ERR_INVALID, "null pointer argument");
    mce_feed_problem q = feed_problem(S1, n1, ld1, S2, n2, ld2, d, cov_mode, kmax, w, fs, dotp, eigenvalues);
    const int rc = mce_evidence_feed_batch_f64(&q, 1, &device, 1);
    if (rc == MCE_OK) *jacobian = q.jacobian;
    return rc;
}

static int feed_part_impl(bool src_device, const double* S1, int64_t n1, int64_t ld1, const double* S2, int64_t n2, int64_t ld2,
                          int32_t d, int32_t cov_mode, int32_t kmax, const double* w, const double* fs,
                          int32_t part, int32_t nparts, double* dotp_part, double* jacobian, double* eigenvalues,
                          uint64_t* checksum, int32_t device)
{
    if (!jacobian) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nparts < 1 || part < 0 || part >= nparts) return fail(MCE_ERR_INVALID, "part %d of %d", part, nparts);
    mce_feed_problem q = feed_problem(S1, n1, ld1, S2, n2, ld2, d, cov_mode, kmax, w, fs, dotp_part, eigenvalues);
    FeedJob job;
    job.part = part;
    job.nparts = nparts;
    return feed_run_one(job, q, src_device, jacobian, checksum, device);
}

int mce_evidence_feed_part_f64(const double* S1, int64_t n1, int64_t ld1, const double* S2, int64_t n2, int64_t ld2,
                               int32_t d, int32_t cov_mode, int32_t kmax, const double* w, const double* fs,
                               int32_t part, int32_t nparts, double* dotp_part, double* jacobian, double* eigenvalues,
                               uint64_t* checksum, int32_t device)
{
    return feed_part_impl(false, S1, n1, ld1, S2, n2, ld2, d, cov_mode, kmax, w, fs, part, nparts, dotp_part, jacobian, eigenvalues, checksum, device);
}

int mce_evidence_feed_part_dev_f64(const double* dS1, int64_t n1, int64_t ld1, const double* dS2, int64_t n2, int64_t ld2,
                                   int32_t d, int32_t cov_mode, int32_t kmax, const double* d_w, const double* d_fs,
                                   int32_t part, int32_t nparts, double* dotp_part, double* jacobian, double* eigenvalues,
                                   uint64_t* checksum, int32_t device)
{
    return feed_part_impl(true, dS1, n1, ld1, dS2, n2, ld2, d, cov_mode, kmax, d_w, d_fs, part, nparts, dotp_part, jacobian, eigenvalues, checksum, device);
}

static int feed_whiten_impl(bool src_device, const double* S1, int64_t n1, int64_t ld1, int32_t d, int32_t kmax, const double* w, const double* fs,
                            double* d_X_out, double* d_w_out, double* d_fs_out, double* jacobian, double* eigenvalues,
                            uint64_t* checksum, int32_t device)
{
    if (!jacobian || !d_X_out || !d_w_out || !d_fs_out) return fail(MCE_ERR_INVALID, "null pointer argument");
    double sums[MCE_MAX_K + 2];
    mce_feed_problem q = feed_problem(S1, n1, ld1, nullptr, 0, 0, d, 0, kmax, w, fs, sums, eigenvalues);
    if (kmax < 2 || kmax > MCE_MAX_K + 1) return fail(MCE_ERR_K_RANGE, "kmax=%d", kmax);
    FeedJob job;
    job.out_X = d_X_out; job.out_w = d_w_out; job.out_f = d_fs_out;
    return feed_run_one(job, q, src_device, jacobian, checksum, device);
}

int mce_evidence_feed_whiten_f64(const double* S1, int64_t n1, int64_t ld1, int32_t d, int32_t kmax, const double* w, const double* fs,
                                 double* d_X_out, double* d_w_out, double* d_fs_out, double* jacobian, double* eigenvalues,
                                 uint64_t* checksum, int32_t device)
{
    return feed_whiten_impl(false, S1, n1, ld1, d, kmax, w, fs, d_X_out, d_w_out, d_fs_out, jacobian, eigenvalues, checksum, device);
}

int mce_evidence_feed_whiten_dev_f64(const double* dS1, int64_t n1, int64_t ld1, int32_t d, int32_t kmax, const double* d_w, const double* d_fs,
                                     double* d_X_out, double* d_w_out, double* d_fs_out, double* jacobian, double* eigenvalues,
                                     uint64_t* checksum, int32_t device)
{
    return feed_whiten_impl(true, dS1, n1, ld1, d, kmax, d_w, d_fs, d_X_out, d_w_out, d_fs_out, jacobian, eigenvalues, checksum, device);
}

int mce_knn_dotp_f64(const double* X, int64_t nq, const double* Y, int64_t nr, int32_t d, int32_t kmax,
                     int32_t k0, int64_t self_offset, const double* w, const double* fs, double* dotp,
                     double* dist_out, const int32_t* devices, int32_t ndev)
{
    if (!X || !Y || !w || !fs || !dotp) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (k0 != 0 && k0 != 1) return fail(MCE_ERR_INVALID, "k0 must be 0 (cross) or 1 (auto), got %d", k0);
    if (kmax <= k0 || nq < 1) return fail(MCE_ERR_INVALID, "invalid kmax=%d k0=%d nq=%lld", kmax, k0, (long long)nq);
    {   // validate before touching any device
        Plan p;
        int rc = make_plan(nq, nr, d, kmax - k0, k0 == 1 ? MCE_SELF_EXCLUDE : MCE_SELF_NONE, p);
        if (rc != MCE_OK) return rc;
    }
    const std::vector<int> devs = device_list(devices, ndev);
    const int n = (int)std::min<int64_t>((int64_t)devs.size(), nq);
    std::vector<std::vector<double>> parts(n, std::vector<double>(kmax, 0.0));
    // auto evidence over one set: let each device take a library-chosen part (rows for the sweep, blocks of the
    // shared k-d order for the pruned walk) instead of a row range
    const bool whole_set = n > 1 && X == Y && nq == nr && k0 == 1 && self_offset == 0 && !dist_out;
    const int rc = for_each_device(devs, n, [&](int i) {
        const int64_t lo = nq * i / n, hi = nq * (i + 1) / n;
        if (whole_set) return mce_knn_dotp_part_f64(Y, nr, d, kmax, i, n, w, fs, parts[i].data(), devs[i]);
        return fused_on_device(devs[i], X, lo, hi, Y, nr, d, kmax, k0, self_offset, w, fs, parts[i].data(), dist_out);
    });
    if (rc != MCE_OK) return rc;
    for (int k = 0; k < kmax; ++k) {   // fixed device order -> reproducible
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += parts[i][k];
        dotp[k] = s;
    }
    return MCE_OK;
}

int mce_knn_dotp_part_f64(const double* Y, int64_t nr, int32_t d, int32_t kmax, int32_t part, int32_t nparts, const double* w,
                          const double* fs, double* dotp, int32_t device)
{
    if (!Y || !w || !fs || !dotp) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (kmax <= 1 || nr < 1) return fail(MCE_ERR_INVALID, "invalid kmax=%d nr=%lld", kmax, (long long)nr);
    Plan p;
    int rc = make_plan(nr, nr, d, kmax - 1, MCE_SELF_EXCLUDE, p);
    if (rc != MCE_OK) return rc;
    rc = select_device(device);
    if (rc != MCE_OK) return rc;
    const size_t wsb = p.total + dotp_ws_bytes(nr, kmax);
    DevBuf dY, dW, dF, dO, ws;
    MCE_HIP(dY.alloc((size_t)nr * d * sizeof(double)));
    MCE_HIP(dW.alloc((size_t)nr * sizeof(double)));
    MCE_HIP(dF.alloc((size_t)nr * sizeof(double)));
    MCE_HIP(dO.alloc((size_t)kmax * sizeof(double)));
    MCE_HIP(ws.alloc(wsb));
    MCE_HIP(hipMemcpy(dY.p, Y, (size_t)nr * d * sizeof(double), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dW.p, w, (size_t)nr * sizeof(double), hipMemcpyHostToDevice));
    MCE_HIP(hipMemcpy(dF.p, fs, (size_t)nr * sizeof(double), hipMemcpyHostToDevice));
    rc = mce_knn_dotp_part_f64_dev(dY.as<double>(), nr, d, kmax, part, nparts, dW.as<double>(), dF.as<double>(), dO.as<double>(), ws.p, wsb, nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipDeviceSynchronize());
    MCE_HIP(hipMemcpy(dotp, dO.p, (size_t)kmax * sizeof(double), hipMemcpyDeviceToHost));
    return MCE_OK;
}

}  // extern "C"
