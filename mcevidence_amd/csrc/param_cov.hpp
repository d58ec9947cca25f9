// param_cov.hpp -- the weighted parameter covariance behind covariance= (the weighted mean and the covariance matrix of the raw
// parameter columns), shared by the host check (tests/native/param_cov_check.cpp, plain C++17 under g++) and the device kernels
// (param_cov_kernels.hpp, __host__ __device__ under hipcc), after the pattern of param_summary.hpp.  docs/design/tension.md states the
// rule; mcevidence_amd/covariance.py (measure) restates it in NumPy.
//
// A SYSTEM is one (x, ld, n, d, w): a_i = w[i], x_ij = x[i * ld + j] for j < d (raw, unwhitened) of the s1 partition the estimator sums
// over.  A row with a_i == 0 is skipped entirely: nothing of it is read into a result.  All in fp64:
//   1  W = sum a,  A2 = sum a^2,  rows = the used count
//   2  m_j = sum a x_j / W
//   3  for i <= j:  C_ij = sum a (x_i - m_i) (x_j - m_j) / W   (a second pass about the COMPUTED m);  C_ji = C_ij is one stored value
// The normalisation is summary's (/ W, no n - 1).  status 3: a weight that is negative or not finite (column -1), else a used row with a
// value that is not finite in a measured column (the lowest such column); status 5: W is not > 0.  With a status other than 0 every value
// is NaN; the used rows stay the count.  The statuses, the row test and their precedence are param_summary.hpp's without the likelihood.
// Here:
//   * cov_tri, cov_tri_doubles             the packed upper triangle, row-major, i <= j (feeders.hpp's indexing);
//   * cov_nblk, cov_nblocks, cov_block     the 16 x 16 blocks of the upper triangle in the order the device deals them out;
//   * cov_term                             one term of the second pass as every route rounds it: (a y_i) y_j;
//   * the result block's layout (kCovHead.., cov_out_doubles, cov_pack_head);
//   * cov_serial                           the serial driver: the whole rule on one CPU thread.
#pragma once

#include <stdint.h>

#include "param_summary.hpp"

#ifndef MCE_COV_HEAD
#define MCE_COV_HEAD 8
#endif

namespace mce_cov {

// the head of a result block
enum : int { kCovW = 0, kCovA2, kCovRows, kCovStatus, kCovColumn, kCovReserved0, kCovReserved1, kCovReserved2, kCovHead };
static_assert(kCovHead == MCE_COV_HEAD, "the result block of include/mcevidence_hip.h");
constexpr int kCovMaxDim = mce_sum::kSumMaxDim;
constexpr int kCovBlock = 16;                                   // columns of a block: one operand of the fp64 MFMA
constexpr int kCovMaxBlocks = 36;                               // nb (nb + 1) / 2 at nb = 8

MCE_HD inline int64_t cov_tri_doubles(int d) { return (int64_t)d * (d + 1) / 2; }
// i <= j < d
MCE_HD inline int64_t cov_tri(int i, int j, int d) { return (int64_t)i * d - (int64_t)i * (i - 1) / 2 + (j - i); }
MCE_HD inline int64_t cov_out_doubles(int d) { return (int64_t)kCovHead + d + cov_tri_doubles(d); }

// column blocks of d columns, and output blocks of their upper triangle
MCE_HD inline int cov_nblk(int d) { return (d + kCovBlock - 1) / kCovBlock; }
MCE_HD inline int cov_nblocks(int d) { return cov_nblk(d) * (cov_nblk(d) + 1) / 2; }
// output block p (row-major over bi <= bj < nb) -> (bi, bj)
MCE_HD inline void cov_block(int p, int nb, int* bi, int* bj)
{
    int i = 0;
    while (p >= nb - i) { p -= nb - i; ++i; }
    *bi = i;
    *bj = i + p;
}

// one term of the second pass: the weight goes to the left factor, then the product
MCE_HD inline double cov_term(double a, double yi, double yj)
{
    const double l = a * yi;
    return l * yj;
}

MCE_HD inline void cov_pack_head(int status, int column, double W, double A2, double rows, double* out)
{
    const bool ok = status == mce_sum::kSumOk;
    const double nan = __builtin_nan("");
    out[kCovW] = ok ? W : nan;
    out[kCovA2] = ok ? A2 : nan;
    out[kCovRows] = rows;
    out[kCovStatus] = (double)status;
    out[kCovColumn] = (double)column;
    out[kCovReserved0] = 0.0;
    out[kCovReserved1] = 0.0;
    out[kCovReserved2] = 0.0;
}

}  // namespace mce_cov

// ---- the serial driver (host): rows in order ------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace mce_cov {

// out: cov_out_doubles(d) doubles
inline void cov_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, double* out)
{
    using namespace mce_sum;
    const double nan = __builtin_nan("");
    double W = 0.0, A2 = 0.0, rows = 0.0;
    bool badw = false;
    int badcol = -1;
    std::vector<int64_t> used;
    for (int64_t i = 0; i < n; ++i) {
        const double a = w[i];
        if (!sum_used(a)) continue;
        used.push_back(i);
        badw = badw || sum_weight_bad(a);
        for (int j = 0; j < d; ++j)
            if (sum_value_bad(x[i * ld + j]) && (badcol < 0 || j < badcol)) badcol = j;
        W += a;
        A2 += a * a;
        rows += 1.0;
    }
    int column;
    const int status = sum_status(badw, false, badcol, W, &column);
    cov_pack_head(status, column, W, A2, rows, out);
    double* mean = out + kCovHead;
    double* cov = mean + d;
    for (int64_t k = 0; k < d + cov_tri_doubles(d); ++k) mean[k] = nan;
    if (status != kSumOk) return;
    for (int j = 0; j < d; ++j) {
        double S = 0.0;
        for (int64_t i : used) S += w[i] * x[i * ld + j];
        mean[j] = S / W;
    }
    std::vector<double> acc((size_t)cov_tri_doubles(d), 0.0), y((size_t)d);
    for (int64_t r : used) {
        for (int j = 0; j < d; ++j) y[(size_t)j] = x[r * ld + j] - mean[j];
        for (int i = 0; i < d; ++i)
            for (int j = i; j < d; ++j) acc[(size_t)cov_tri(i, j, d)] += cov_term(w[r], y[(size_t)i], y[(size_t)j]);
    }
    for (int64_t k = 0; k < cov_tri_doubles(d); ++k) cov[k] = acc[(size_t)k] / W;
}

}  // namespace mce_cov
#endif
