// capi_eig.hpp -- part of capi.hip: the batched symmetric eigen-solver's launch (eig_kernels.hpp), the choice between the host
// and the device solver of the evidence feed (mce_options.eig_mode, MCE_FEED_EIG), the counters behind mce_last_eig_stats, and
// the two entry points that reach both solvers directly.
#pragma once
namespace {

using mce_eig::jacobi_eig;

// 1 host (jacobi_eig between two waits, as always), 2 device (eig_jacobi_kernel on the job's stream)
int eff_eig_mode() { return t_opt.eig > 0 ? t_opt.eig : env_feed_eig(); }

// what the calling thread's last feed call solved: systems on the device / on the host, and of the device solves the largest
// number of sweeps and the rotations in all (the host solver does not count its own)
struct EigStats { double dev = 0, host = 0, sweeps = 0, rotations = 0; };
thread_local EigStats g_eig_stats;
void eig_stats_add(EigStats& s, const int32_t* stat)
{
    s.dev += 1;
    s.sweeps = std::max(s.sweeps, (double)stat[mce_eig::kStatSweeps]);
    s.rotations += (double)stat[mce_eig::kStatRotations];
}
void eig_stats_merge(EigStats& s, const EigStats& o)
{
    s.dev += o.dev;
    s.host += o.host;
    s.sweeps = std::max(s.sweeps, o.sweeps);
    s.rotations += o.rotations;
}

// a solve's status in the feed's words (the host solver's: feed_eig_system)
int eig_status_fail(const int32_t* stat, const double* lam)
{
    if (stat[mce_eig::kStatCode] == mce_eig::kStatusNotFinite) return fail(MCE_ERR_INVALID, "samples contain NaN or infinity (non-finite covariance)");
    const int i = stat[mce_eig::kStatIndex];
    return fail(MCE_ERR_INVALID, "math domain error: covariance eigenvalue %d is %g (use fewer parameters, ndim)", i, lam[i]);
}

// the solver stages the whole matrix in LDS (up to 133 KB): raise the dynamic limit once per device
int eig_attr_once()
{
    static std::atomic<bool> attr_set[kMaxDevices];
    int dev = 0;
    MCE_HIP(hipGetDevice(&dev));
    if (dev < kMaxDevices && !attr_set[dev].load()) {
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::eig_jacobi_kernel<16, 256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mce::eig_lds_bytes(mce::kEigNarrowDim)));
        MCE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mce::eig_jacobi_kernel<8, 1024>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mce::eig_lds_bytes(mce::kEigMaxDim)));
        attr_set[dev].store(true);
    }
    return MCE_OK;
}
static_assert(mce::eig_lds_bytes(mce::kEigMaxDim) <= 160 * 1024, "the matrix of the largest system fits a CU's LDS");

// nsys systems, one workgroup each; enqueue only
int launch_eig(const double* d_cov, int d, int64_t nsys, double* d_evec, double* d_scale, double* d_lam, int32_t* d_status, hipStream_t st)
{
    int rc = eig_attr_once();
    if (rc != MCE_OK) return rc;
    if (d <= mce::kEigNarrowDim)
        hipLaunchKernelGGL((mce::eig_jacobi_kernel<16, 256>), dim3((unsigned)nsys), dim3(mce::eig_threads(d)), mce::eig_lds_bytes(d), st, d_cov, d, d_evec,
                           d_scale, d_lam, d_status);
    else
        hipLaunchKernelGGL((mce::eig_jacobi_kernel<8, 1024>), dim3((unsigned)nsys), dim3(mce::eig_threads(d)), mce::eig_lds_bytes(d), st, d_cov, d, d_evec,
                           d_scale, d_lam, d_status);
    MCE_HIP(hipGetLastError());
    return MCE_OK;
}

int eig_batch_check(const void* a, const void* b, const void* c, const void* e, const void* f, int32_t d, int64_t nsys)
{
    if (!a || !b || !c || !e || !f) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (d < 1 || nsys < 1 || nsys > INT32_MAX) return fail(MCE_ERR_INVALID, "invalid sizes d=%d nsys=%lld", d, (long long)nsys);
    if (d > mce::kEigMaxDim) return fail(MCE_ERR_DIM_RANGE, "the batched eigen-solver supports d <= %d (got %d)", mce::kEigMaxDim, d);
    return MCE_OK;
}

}  // namespace

extern "C" {

int mce_eig_sym_batch_dev_f64(const double* d_cov, int32_t d, int64_t nsys, double* d_evec, double* d_scale, double* d_lam, int32_t* d_status, void* stream)
{
    const int rc = eig_batch_check(d_cov, d_evec, d_scale, d_lam, d_status, d, nsys);
    if (rc != MCE_OK) return rc;
    return launch_eig(d_cov, d, nsys, d_evec, d_scale, d_lam, d_status, static_cast<hipStream_t>(stream));
}

int mce_eig_sym_batch_f64(const double* cov, int32_t d, int64_t nsys, int32_t mode, double* evec, double* scale, double* lam, int32_t* status, int32_t device)
{
    int rc = eig_batch_check(cov, evec, scale, lam, status, d, nsys);
    if (rc != MCE_OK) return rc;
    if (mode != 1 && mode != 2) return fail(MCE_ERR_INVALID, "mode must be 1 (host solver) or 2 (device solver), got %d", mode);
    const size_t dd = (size_t)d * d;
    if (mode == 1) {
        for (int64_t i = 0; i < nsys; ++i) {
            std::vector<double> A(cov + i * dd, cov + (i + 1) * dd), l((size_t)d), V(dd, 0.0);
            bool finite = true;
            for (double x : A) finite = finite && mce_eig::is_finite(x);
            int32_t* st = status + i * mce_eig::kStatInts;
            int index = 0;
            if (finite) {
                jacobi_eig(A, d, l, V);
                st[mce_eig::kStatCode] = mce_eig::status_of(l.data(), d, index);
            } else {                                                             // as the device solver: the input's diagonal, no sweep
                for (int r = 0; r < d; ++r) l[r] = A[(size_t)r * d + r];
                st[mce_eig::kStatCode] = mce_eig::kStatusNotFinite;
            }
            st[mce_eig::kStatIndex] = index;
            st[mce_eig::kStatSweeps] = st[mce_eig::kStatRotations] = 0;          // (not counted by the host solver)
            const bool ok = st[mce_eig::kStatCode] == mce_eig::kStatusOk;
            for (int r = 0; r < d; ++r) {
                for (int c = 0; c < d; ++c) evec[i * dd + (size_t)r * d + c] = ok ? V[(size_t)r * d + c] : (r == c ? 1.0 : 0.0);
                lam[i * d + r] = l[r];
                scale[i * d + r] = ok ? 1.0 / std::sqrt(l[r]) : 1.0;
            }
        }
        return MCE_OK;
    }
    rc = select_device(device);
    if (rc != MCE_OK) return rc;
    DevBuf dC, dV, dS, dL, dT;
    MCE_HIP(dC.alloc(nsys * dd * sizeof(double)));
    MCE_HIP(dV.alloc(nsys * dd * sizeof(double)));
    MCE_HIP(dS.alloc((size_t)nsys * d * sizeof(double)));
    MCE_HIP(dL.alloc((size_t)nsys * d * sizeof(double)));
    MCE_HIP(dT.alloc((size_t)nsys * mce_eig::kStatInts * sizeof(int32_t)));
    MCE_HIP(hipMemcpy(dC.p, cov, nsys * dd * sizeof(double), hipMemcpyHostToDevice));
    rc = launch_eig(dC.as<double>(), d, nsys, dV.as<double>(), dS.as<double>(), dL.as<double>(), dT.as<int32_t>(), nullptr);
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipDeviceSynchronize());
    MCE_HIP(hipMemcpy(evec, dV.p, nsys * dd * sizeof(double), hipMemcpyDeviceToHost));
    MCE_HIP(hipMemcpy(scale, dS.p, (size_t)nsys * d * sizeof(double), hipMemcpyDeviceToHost));
    MCE_HIP(hipMemcpy(lam, dL.p, (size_t)nsys * d * sizeof(double), hipMemcpyDeviceToHost));
    MCE_HIP(hipMemcpy(status, dT.p, (size_t)nsys * mce_eig::kStatInts * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MCE_OK;
}

int mce_last_eig_stats(double* out, int32_t n)
{
    if (!out || n < 4) return fail(MCE_ERR_INVALID, "mce_last_eig_stats: out[4] expected");
    out[0] = g_eig_stats.dev;
    out[1] = g_eig_stats.host;
    out[2] = g_eig_stats.sweeps;
    out[3] = g_eig_stats.rotations;
    return MCE_OK;
}

}  // extern "C"
