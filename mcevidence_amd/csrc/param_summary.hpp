// param_summary.hpp -- the posterior summary behind summary= (weighted means, variances, extremes, weighted quantiles and the best-fit
// sample of the parameter columns), shared by the host check (tests/native/param_summary_check.cpp, plain C++17 under g++) and the
// device kernels (param_summary_kernels.hpp, __host__ __device__ under hipcc), after the pattern of like_moments.hpp.
// docs/design/summary.md states the rule; mcevidence_amd/summary.py (measure) restates it in NumPy.
//
// A SYSTEM is one (x, ld, n, d, w, fs): a_i = w[i], x_ij = x[i * ld + j] for j < d (raw, unwhitened), f_i = fs[i] of the s1 partition
// the estimator sums over.  A row with a_i == 0 is skipped entirely: nothing of it is read into a result.  All in fp64:
//   1  W = sum a,  A2 = sum a^2
//   2  m_j = sum a x_j / W,   v_j = sum a (x_j - m_j)^2 / W   (a second pass about the COMPUTED m_j),   min_j, max_j over used rows
//   3  Q_j(q) = the smallest x among the used rows with C_j(x) >= q * W, C_j(x) = sum of a over used rows with x_ij <= x: the used rows
//      in a stable sort by x_j, a accumulated in that order, the value at the first position whose running sum reaches q * W (one
//      fp64 product); where rounding keeps every running sum below it, the last position.  No interpolation.
//   4  best fit: the used row with the largest f, the lowest row among equals; f = -inf is a legal value
// status 3: a weight that is negative or not finite (column -1), else a used row whose f is NaN (column -2), else a used row with a
// value that is not finite in a measured column (the lowest such column); status 5: W is not > 0.  With a status other than 0 every
// value is NaN; the used rows stay the count.
// Here:
//   * sum_used, sum_weight_bad, sum_value_bad, sum_like_bad      the row test and what status 3 refuses;
//   * sum_status                                                 the precedence of the statuses;
//   * sum_key, sum_unkey                                         the order-preserving 64-bit key of a double and its inverse
//                                                                (-0.0 takes +0.0's key: equal values, one key);
//   * sum_term                                                   a (x - m)^2 as every route rounds it;
//   * sum_search                                                 the quantile search on a sorted run;
//   * sum_better                                                 the order of the best-fit pairs;
//   * the result block's layout (kSumHead.., sum_out_doubles, sum_pack_head);
//   * sum_serial                                                 the serial driver: the whole rule on one CPU thread.
#pragma once

#include <stdint.h>
#include <string.h>

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

#ifndef MCE_SUMMARY_MAX_Q
#define MCE_SUMMARY_MAX_Q 16
#endif
#ifndef MCE_SUMMARY_HEAD
#define MCE_SUMMARY_HEAD 8
#endif

namespace mce_sum {

enum : int {
    kSumOk = 0,
    kSumNotFinite = 3,       // a bad weight, a NaN likelihood of a used row, or a value that is not finite in a used row
    kSumNoWeight = 5         // W is not > 0 (this covers a system without a used row)
};
enum : int { kSumColNone = -1, kSumColLike = -2 };
// the head of a result block
enum : int { kSumW = 0, kSumA2, kSumRows, kSumStatus, kSumColumn, kSumBestRow, kSumBestF, kSumReserved, kSumHead };
static_assert(kSumHead == MCE_SUMMARY_HEAD, "the result block of include/mcevidence_hip.h");
// the per-column rows after the head: d doubles each, then nq quantile rows
enum : int { kSumMean = 0, kSumVar, kSumMin, kSumMax, kSumBest, kSumPerCol };
constexpr int kSumMaxDim = 127;

MCE_HD inline int64_t sum_out_doubles(int d, int nq) { return (int64_t)kSumHead + (int64_t)d * (kSumPerCol + nq); }

MCE_HD inline bool sum_finite(double x) { return x - x == 0.0; }
// a NaN weight is "used": it is what status 3 reports
MCE_HD inline bool sum_used(double a) { return !(a == 0.0); }
// of a used row
MCE_HD inline bool sum_weight_bad(double a) { return !sum_finite(a) || a < 0.0; }
MCE_HD inline bool sum_value_bad(double x) { return !sum_finite(x); }
MCE_HD inline bool sum_like_bad(double f) { return f != f; }

// badw, badf: a used row with a bad weight / a NaN f was seen; badcol: the lowest column with a bad value, or -1
MCE_HD inline int sum_status(bool badw, bool badf, int badcol, double W, int* column)
{
    *column = kSumColNone;
    if (badw) return kSumNotFinite;
    if (badf) { *column = kSumColLike; return kSumNotFinite; }
    if (badcol >= 0) { *column = badcol; return kSumNotFinite; }
    return !(W > 0.0) ? kSumNoWeight : kSumOk;
}

// unsigned order of the keys == numerical order of the doubles; -0.0 and +0.0 are one value and get one key
MCE_HD inline uint64_t sum_key(double x)
{
    uint64_t u;
    if (x == 0.0) x = 0.0;
    memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
MCE_HD inline double sum_unkey(uint64_t k)
{
    const uint64_t u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
    double x;
    memcpy(&x, &u, 8);
    return x;
}
// what a row that is not used is given on the device: it sorts behind every used row and adds nothing
constexpr uint64_t kSumPadKey = ~(uint64_t)0;

// one term of the second pass: the difference, its square, the product
MCE_HD inline double sum_term(double a, double x, double m)
{
    const double d = x - m;
    const double s = d * d;
    return a * s;
}

// the first position p in [p0, p1) whose running sum, started at `base` and taking a[p0], a[p0 + 1], .. in turn, reaches `target`;
// p1 where none does.  *running is left at the sum at the returned position (or over the whole range).
MCE_HD inline int64_t sum_search(const double* a, int64_t p0, int64_t p1, double base, double target, double* running)
{
    double run = base;
    for (int64_t p = p0; p < p1; ++p) {
        run += a[p];
        if (run >= target) { *running = run; return p; }
    }
    *running = run;
    return p1;
}

// does (f, row) beat the best (bf, brow) so far?  (brow < 0: there is none yet)
MCE_HD inline bool sum_better(double f, int64_t row, double bf, int64_t brow)
{
    if (row < 0) return false;
    if (brow < 0) return true;
    return f > bf || (f == bf && row < brow);
}

MCE_HD inline void sum_pack_head(int status, int column, double W, double A2, double rows, int64_t best_row, double best_f, double* out)
{
    const bool ok = status == kSumOk;
    const double nan = __builtin_nan("");
    out[kSumW] = ok ? W : nan;
    out[kSumA2] = ok ? A2 : nan;
    out[kSumRows] = rows;
    out[kSumStatus] = (double)status;
    out[kSumColumn] = (double)column;
    out[kSumBestRow] = ok ? (double)best_row : -1.0;
    out[kSumBestF] = (ok && best_row >= 0) ? best_f : nan;
    out[kSumReserved] = 0.0;
}

}  // namespace mce_sum

// ---- the serial driver (host): rows in order ------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>

namespace mce_sum {

// out: sum_out_doubles(d, nq) doubles.  fs may be null: no best fit.
inline void sum_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const double* fs, const double* q, int nq, double* out)
{
    const double nan = __builtin_nan("");
    double W = 0.0, A2 = 0.0, rows = 0.0;
    bool badw = false, badf = false;
    int badcol = -1;
    int64_t brow = -1;
    double bf = 0.0;
    std::vector<int64_t> used;
    for (int64_t i = 0; i < n; ++i) {
        const double a = w[i];
        if (!sum_used(a)) continue;
        used.push_back(i);
        badw = badw || sum_weight_bad(a);
        if (fs) {
            badf = badf || sum_like_bad(fs[i]);
            if (sum_better(fs[i], i, bf, brow)) { bf = fs[i]; brow = i; }
        }
        for (int j = 0; j < d; ++j)
            if (sum_value_bad(x[i * ld + j]) && (badcol < 0 || j < badcol)) badcol = j;
        W += a;
        A2 += a * a;
        rows += 1.0;
    }
    int column;
    const int status = sum_status(badw, badf, badcol, W, &column);
    sum_pack_head(status, column, W, A2, rows, brow, bf, out);
    double* col = out + kSumHead;
    const int64_t total = (int64_t)d * (kSumPerCol + nq);
    for (int64_t k = 0; k < total; ++k) col[k] = nan;
    if (status != kSumOk) return;
    std::vector<int64_t> order(used.size());
    std::vector<double> as(used.size());
    for (int j = 0; j < d; ++j) {
        double S = 0.0, mn = HUGE_VAL, mx = -HUGE_VAL;
        for (int64_t i : used) {
            const double v = x[i * ld + j];
            S += w[i] * v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        const double m = S / W;
        double V = 0.0;
        for (int64_t i : used) V += sum_term(w[i], x[i * ld + j], m);
        col[kSumMean * d + j] = m;
        col[kSumVar * d + j] = V / W;
        col[kSumMin * d + j] = sum_unkey(sum_key(mn));
        col[kSumMax * d + j] = sum_unkey(sum_key(mx));
        if (brow >= 0) col[kSumBest * d + j] = x[brow * ld + j];
        order = used;
        std::stable_sort(order.begin(), order.end(), [&](int64_t p, int64_t r) { return sum_key(x[p * ld + j]) < sum_key(x[r * ld + j]); });
        for (size_t k = 0; k < order.size(); ++k) as[k] = w[order[k]];
        for (int t = 0; t < nq; ++t) {
            double run;
            int64_t p = sum_search(as.data(), 0, (int64_t)as.size(), 0.0, q[t] * W, &run);
            if (p >= (int64_t)as.size()) p = (int64_t)as.size() - 1;
            col[(kSumPerCol + t) * d + j] = sum_unkey(sum_key(x[order[(size_t)p] * ld + j]));
        }
    }
}

}  // namespace mce_sum
#endif
