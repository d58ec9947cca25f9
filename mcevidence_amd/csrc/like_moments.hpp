// like_moments.hpp -- the weighted moments of the likelihood column behind information= (<ln L>_P, Var_P(ln L), N_eff), shared by the
// host check (tests/native/like_moments_check.cpp, plain C++17 under g++) and the device kernels (like_moments_kernels.hpp,
// __host__ __device__ under hipcc), after the pattern of jack.hpp and chain_conv.hpp.  docs/design/information.md states the rule;
// mcevidence_amd/information.py (moments) restates it in NumPy.
//
// A SYSTEM is one (fs, w, n): a_i = w[i], f_i = fs[i] = logL_i - logLmax of the s1 partition the estimator sums over.  A row with
// a_i == 0 is skipped entirely: its f_i is never read into a sum.  All in fp64:
//   1  W = sum a,   S = sum a f,   A2 = sum a^2,   c = S / W
//   2  v = sum a (f - c)^2 / W                     (a second pass, centred on the COMPUTED c; never sum a f^2 - ..)
// status 3: a weight that is not finite, or a row with a != 0 whose f is not finite (-inf included); status 5: W is not > 0 (no row
// left included).  Negative weights are allowed, as in the estimator.  With a status other than 0 every value is NaN.
// Here:
//   * mom_used, mom_row_bad          the row test and what status 3 refuses;
//   * mom_status                     the precedence of the statuses: 3, then 5;
//   * mom_term                       a (f - c)^2 as every route rounds it: three roundings;
//   * mom_pack                       the result block of a system: W, c, v, A2, rows used, status;
//   * mom_serial                     the serial driver: the whole rule on one CPU thread.
#pragma once

#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef MCE_HD
#define MCE_HD __host__ __device__
#endif
#else
#ifndef MCE_HD
#define MCE_HD
#endif
#endif

#ifndef MCE_MOMENTS_OUT
#define MCE_MOMENTS_OUT 6
#endif

namespace mce_mom {

enum : int {
    kMomOk = 0,
    kMomNotFinite = 3,       // a weight that is not finite, or a used row whose f is not finite
    kMomNoWeight = 5         // W is not > 0 (this covers a system without a used row)
};
enum : int { kMomW = 0, kMomC, kMomV, kMomA2, kMomRows, kMomStatus, kMomOut };
static_assert(kMomOut == MCE_MOMENTS_OUT, "the result block of include/mcevidence_hip.h");

MCE_HD inline bool mom_finite(double x) { return x - x == 0.0; }
// a NaN weight is "used": it is what status 3 reports
MCE_HD inline bool mom_used(double a) { return !(a == 0.0); }
// of a used row
MCE_HD inline bool mom_row_bad(double a, double f) { return !mom_finite(a) || !mom_finite(f); }

MCE_HD inline int mom_status(bool bad, double W) { return bad ? kMomNotFinite : (!(W > 0.0) ? kMomNoWeight : kMomOk); }

// one term of step 2: the difference, its square, the product -- in this order (a compiler may fuse the product into the caller's
// sum: one rounding fewer, never one more)
MCE_HD inline double mom_term(double a, double f, double c)
{
    const double d = f - c;
    const double q = d * d;
    return a * q;
}

MCE_HD inline void mom_pack(int status, double W, double c, double v, double A2, double rows, double* out)
{
    const bool ok = status == kMomOk;
    const double nan = __builtin_nan("");
    out[kMomW] = ok ? W : nan;
    out[kMomC] = ok ? c : nan;
    out[kMomV] = ok ? v : nan;
    out[kMomA2] = ok ? A2 : nan;
    out[kMomRows] = rows;
    out[kMomStatus] = (double)status;
}

// ---- the serial driver (host): rows in order ------------------------------------------------------------------------------------
inline void mom_serial(const double* fs, const double* w, int64_t n, double* out)
{
    double W = 0.0, S = 0.0, A2 = 0.0, rows = 0.0;
    bool bad = false;
    for (int64_t i = 0; i < n; ++i) {
        const double a = w[i];
        if (!mom_used(a)) continue;
        const double f = fs[i];
        bad = bad || mom_row_bad(a, f);
        W += a;
        S += a * f;
        A2 += a * a;
        rows += 1.0;
    }
    const int status = mom_status(bad, W);
    const double c = S / W;
    double V = 0.0;
    if (status == kMomOk)
        for (int64_t i = 0; i < n; ++i)
            if (mom_used(w[i])) V += mom_term(w[i], fs[i], c);
    mom_pack(status, W, c, V / W, A2, rows, out);
}

}  // namespace mce_mom
