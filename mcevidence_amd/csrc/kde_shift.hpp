// kde_shift.hpp -- the non-Gaussian parameter shift behind shift="kde" (--shift-kde): a leave-one-out Gaussian kernel density estimate
// on the whitened rows of a parameter-DIFFERENCE chain and the posterior mass above the density at a point (Raveri & Doux,
// arXiv:2105.03324), shared by the host check (tests/native/kde_shift_check.cpp, plain C++17 under g++) and the device kernels
// (kde_kernels.hpp, __host__ __device__ under hipcc), after the pattern of param_cov.hpp.  docs/design/shift_kde.md states the rule;
// mcevidence_amd/shift_kde.py (measure) restates it in NumPy.
//
// A SYSTEM is one (x, ld, n, d, w, linv, mean, point, c): w_i = w[i], x_ij = x[i * ld + j] for j < d, linv the row-major lower
// triangle L^-1 of the covariance's Cholesky factor (entries above the diagonal are not read), c = 1 / (2 h^2).  A row with w_i == 0 is
// skipped entirely: nothing of it is read into a result.  All in fp64:
//   1  W = sum w,  A2 = sum w^2,  rows = the used count
//   2  z_ik = sum_{j <= k} linv_kj (x_ij - mean_j)   (plain products and sums in column order),   z_0 likewise from `point`
//   3  for a used row i:  S_i = sum over used j != i of w_j exp(-c max(0, |z_i|^2 + |z_j|^2 - 2 z_i . z_j)),   t_i = S_i / (W - w_i);
//      here and in 4 a kernel value whose argument is at or above kKdeUnderflow = 746 is +0.0
//   4  at the point, over all used j:  K_0j = exp(-c |z_0 - z_j|^2) (the differences squared, in column order),  S_0 = sum w_j K_0j,
//      Q_0 = sum w_j^2 K_0j^2,  t_0 = S_0 / W,  s_0 = sqrt(Q_0) / W
//   5  M(tau) = sum over used i of w_i [t_i > tau] at tau = t_0, t_0 - s_0, t_0 + s_0;   M_eq = sum w_i [t_i == t_0]
// status 3: a weight that is negative or not finite; 4: a used row with a value that is not finite in a measured column (column: the
// lowest such); 5: W is not > 0; 6: fewer than 2 used rows -- in that precedence.  With a status other than 0 every value is NaN; the
// used rows stay the count.  (Status 7, a covariance that is not positive definite, is the caller's: it has no linv to hand over.)
// Here:
//   * kde_whiten_coord, kde_dist2, kde_point_dist2, kde_kernel_term     the pieces as every route rounds them;
//   * kde_nchunks, kde_nparts, kde_part_chunk                           how the device cuts a system's reference rows: by n alone;
//   * kde_status, the result block's layout (kKde.., kKdeOut, kde_pack);
//   * kde_serial                                                        the serial driver: the whole rule on one CPU thread.
#pragma once

#include <stdint.h>

#include <cmath>

#include "param_summary.hpp"

#ifndef MCE_KDE_OUT
#define MCE_KDE_OUT 16
#endif
#ifndef MCE_KDE_MAX_DIM
#define MCE_KDE_MAX_DIM 64
#endif

namespace mce_kde {

enum : int { kKdeOk = 0, kKdeBadWeight = 3, kKdeBadValue = 4, kKdeNoWeight = 5, kKdeFewRows = 6 };
// the result block of a system
enum : int { kKdeW = 0, kKdeA2, kKdeRows, kKdeStatus, kKdeColumn, kKdeC, kKdeS0, kKdeQ0, kKdeM0, kKdeMlo, kKdeMhi, kKdeMeq, kKdeOut = 16 };
static_assert(kKdeOut == MCE_KDE_OUT, "the result block of include/mcevidence_hip.h");
constexpr int kKdeMaxDim = MCE_KDE_MAX_DIM;
constexpr int kKdeChunkRows = 64;                               // reference rows staged at a time, and the query rows of a workgroup
constexpr int kKdeMaxParts = 8;                                 // parts of a system's reference range
// THE RULE takes a kernel value whose argument c D is at or above this as +0.0: its exact value is below 0.17 * 2^-1074, so a correctly
// rounded exp gives +0.0 there anyway, and no route depends on what its exp routine returns that far down.  It is what lets the device
// skip a 16 x 16 tile of such arguments without changing a bit.
constexpr double kKdeUnderflow = 746.0;

// the column count padded to whole k-steps of the fp64 MFMA
MCE_HD inline int kde_dpad(int d) { return (d + 3) & ~3; }
MCE_HD inline int64_t kde_nchunks(int64_t n) { return (n + kKdeChunkRows - 1) / kKdeChunkRows; }
MCE_HD inline int kde_nparts(int64_t n)
{
    const int64_t c = kde_nchunks(n);
    return c < 1 ? 1 : (c < kKdeMaxParts ? (int)c : kKdeMaxParts);
}
// the first chunk of part p (p = nparts: the end)
MCE_HD inline int64_t kde_part_chunk(int64_t n, int p) { return kde_nchunks(n) * p / kde_nparts(n); }

// coordinate k of a whitened row: y_j = x_j - mean_j, the products added in column order
MCE_HD inline double kde_whiten_coord(const double* lrow, const double* x, const double* mean, int k)
{
    double acc = 0.0;
    for (int j = 0; j <= k; ++j) {
        const double y = x[j] - mean[j];
        const double p = lrow[j] * y;
        acc = acc + p;
    }
    return acc;
}

// the squared distance of a pair from the norms and the dot product, never negative
MCE_HD inline double kde_dist2(double qn, double zn, double dot)
{
    const double s = qn + zn;
    const double D = s - 2.0 * dot;
    return D > 0.0 ? D : 0.0;
}

// one term of a sum: w exp(-c D)
MCE_HD inline double kde_kernel_arg_value(double arg) { return arg >= kKdeUnderflow ? 0.0 : exp(-arg); }
MCE_HD inline double kde_kernel_value(double c, double D) { return kde_kernel_arg_value(c * D); }

MCE_HD inline int kde_status(bool badw, int badcol, double W, double rows, int* column)
{
    *column = -1;
    if (badw) return kKdeBadWeight;
    if (badcol >= 0) { *column = badcol; return kKdeBadValue; }
    if (!(W > 0.0)) return kKdeNoWeight;
    return rows < 2.0 ? kKdeFewRows : kKdeOk;
}

// M[4]: M(t0), M(t0 - s0), M(t0 + s0), M_eq
MCE_HD inline void kde_pack(int status, int column, double W, double A2, double rows, double c, double S0, double Q0, const double* M, double* out)
{
    const bool ok = status == kKdeOk;
    const double nan = __builtin_nan("");
    out[kKdeW] = ok ? W : nan;
    out[kKdeA2] = ok ? A2 : nan;
    out[kKdeRows] = rows;
    out[kKdeStatus] = (double)status;
    out[kKdeColumn] = (double)column;
    out[kKdeC] = ok ? c : nan;
    out[kKdeS0] = ok ? S0 : nan;
    out[kKdeQ0] = ok ? Q0 : nan;
    for (int k = 0; k < 4; ++k) out[kKdeM0 + k] = ok ? M[k] : nan;
    for (int k = kKdeMeq + 1; k < kKdeOut; ++k) out[k] = 0.0;
}

// the selection sums' tests of one used row
MCE_HD inline void kde_select(double t, double w, double t0, double s0, double* M)
{
    M[0] += t > t0 ? w : 0.0;
    M[1] += t > t0 - s0 ? w : 0.0;
    M[2] += t > t0 + s0 ? w : 0.0;
    M[3] += t == t0 ? w : 0.0;
}

}  // namespace mce_kde

// ---- the serial driver (host): rows in order ------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace mce_kde {

// out: kKdeOut doubles; dens: null or n + 1 doubles (t_i, NaN for a row that is not used, t_0 last); zout: null or n * d doubles
inline void kde_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const double* linv, const double* mean, const double* point, double c,
                       double* out, double* dens, double* zout)
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
    const int status = kde_status(badw, badcol, W, rows, &column);
    double M[4] = {0.0, 0.0, 0.0, 0.0};
    if (dens) for (int64_t i = 0; i <= n; ++i) dens[i] = nan;
    if (zout) for (int64_t i = 0; i < n * d; ++i) zout[i] = 0.0;
    if (status != kKdeOk) {
        kde_pack(status, column, W, A2, rows, c, nan, nan, M, out);
        return;
    }
    const size_t m = used.size(), D = (size_t)d;
    std::vector<double> z(m * D), zn(m), z0(D), t(m);
    for (int k = 0; k < d; ++k) z0[(size_t)k] = kde_whiten_coord(linv + (size_t)k * D, point, mean, k);
    double S0 = 0.0, Q0 = 0.0;
    for (size_t u = 0; u < m; ++u) {
        const double* xr = x + used[u] * ld;
        double nn = 0.0, d0 = 0.0;
        for (int k = 0; k < d; ++k) {
            const double v = kde_whiten_coord(linv + (size_t)k * D, xr, mean, k);
            z[u * D + (size_t)k] = v;
            if (zout) zout[used[u] * d + k] = v;
            nn += v * v;
            const double e = v - z0[(size_t)k];
            d0 += e * e;
        }
        zn[u] = nn;
        const double wk = w[used[u]] * kde_kernel_value(c, d0);
        S0 += wk;
        Q0 += wk * wk;
    }
    for (size_t u = 0; u < m; ++u) {
        double S = 0.0;
        for (size_t v = 0; v < m; ++v) {
            if (v == u) continue;
            double dot = 0.0;
            for (size_t k = 0; k < D; ++k) dot += z[u * D + k] * z[v * D + k];
            S += w[used[v]] * kde_kernel_value(c, kde_dist2(zn[u], zn[v], dot));
        }
        t[u] = S / (W - w[used[u]]);
    }
    const double t0 = S0 / W, s0 = sqrt(Q0) / W;
    for (size_t u = 0; u < m; ++u) {
        kde_select(t[u], w[used[u]], t0, s0, M);
        if (dens) dens[used[u]] = t[u];
    }
    if (dens) dens[n] = t0;
    kde_pack(status, column, W, A2, rows, c, S0, Q0, M, out);
}

}  // namespace mce_kde
#endif
