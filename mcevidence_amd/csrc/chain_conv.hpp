// chain_conv.hpp -- the Gelman-Rubin statistic "R-1" of a set of chains (converge=), shared by the host check
// (tests/native/chain_conv_check.cpp, plain C++17 under g++) and the device kernels (chain_conv_kernels.hpp, __host__ __device__ under
// hipcc), after the pattern of chain_corr.hpp and jack.hpp.  docs/design/chain_conv.md states the rule; mcevidence_amd/chains.py
// (gelman_rubin) restates it in NumPy.
//
// A SEGMENT is a run of rows of one burned chain (a whole part, or a half of one); a segment without rows or of total weight 0 is
// skipped; M segments are left (M >= 2).  With w the raw weights and x_j the first ndim parameter columns, all in fp64:
//   1  c_j      = sum w x_j / sum w over all segments             (a centre only)
//   2  W_s      = sum_s w,   a_sj = sum_s w (x_j - c_j) / W_s
//   3  o_j      = sum_s W_s a_sj / sum_s W_s,   delta_sj = a_sj - o_j
//   4  C_s[i][j] = sum_s w (x_i - c_i - a_si)(x_j - c_j - a_sj) / W_s
//   5  Wc = sum_s C_s / M,   B = sum_s delta_s delta_s^T / (M - 1)
//   6  sigma_j = sqrt(Wc[j][j]),   per_param[j] = B[j][j] / Wc[j][j]
//   7  Wn = Wc / (sigma sigma^T) = U Lambda U^T
//   8  v_s = Lambda^(-1/2) U^T (delta_s / sigma),   T = sum_s v_s v_s^T / (M - 1),   r_minus_1 = lambda_max(T) = lambda_max(T + I) - 1
// Here:
//   * conv_weight_ok, conv_value_ok      what status 3 refuses;
//   * conv_posdef                        what status 4 refuses;
//   * conv_pair                          the packed index of (i <= j) of a d x d symmetric matrix, row-major upper triangle;
//   * conv_status                        the precedence of the statuses: 3, 5, 2 (4 comes from the solver afterwards);
//   * conv_serial                        the serial driver: the whole rule on one CPU thread (eig_jacobi.hpp's tournament solver).
#pragma once

#include "eig_jacobi.hpp"

#include <cmath>
#include <cstdint>
#include <utility>
#include <vector>

#ifndef MCE_CONV_MAX_SEGMENTS
#define MCE_CONV_MAX_SEGMENTS 128
#endif

namespace mce_conv {

enum : int {
    kConvOk = 0,
    kConvConstant = 2,       // Wc[j][j] is not > 0
    kConvNotFinite = 3,      // a value of a measured column that is not finite (column j), or a weight that is negative or not finite (column -1)
    kConvNotPositive = 4,    // Wn is not positive definite (the solver's code 2)
    kConvFewSegments = 5     // fewer than 2 segments with rows and weight (seen only once the weights are summed)
};
constexpr int kConvMaxDim = 127;
constexpr int kConvMaxSegments = MCE_CONV_MAX_SEGMENTS;

MCE_HD inline bool conv_weight_ok(double w) { return w >= 0.0 && w - w == 0.0; }
MCE_HD inline bool conv_value_ok(double v) { return v - v == 0.0; }

// Wn counts as positive definite when the solver says so AND its smallest eigenvalue clears the solver's own absolute error, taken as
// 64 d eps (the trace of Wn is d): a singular Wn comes out of fp64 with eigenvalues of either sign around 0, and a sign must not decide
constexpr double kConvPdTol = 64.0 * 2.220446049250313e-16;
MCE_HD inline bool conv_posdef(int solver_code, double lam_min, int d) { return solver_code == mce_eig::kStatusOk && lam_min > kConvPdTol * (double)d; }

MCE_HD inline int conv_npair(int d) { return d * (d + 1) / 2; }
MCE_HD inline int conv_pair(int d, int i, int j) { return i * d - i * (i - 1) / 2 + (j - i); }

// status before the solver: bad_weight, then the lowest column with a value that is not finite (bad_col[j] != 0), then too few
// segments, then the lowest column whose Wc[j][j] (diag[j]) is not > 0
MCE_HD inline int conv_status(bool bad_weight, const int* bad_col, int used, const double* diag, int d, int* column)
{
    if (bad_weight) { *column = -1; return kConvNotFinite; }
    for (int j = 0; j < d; ++j)
        if (bad_col[j]) { *column = j; return kConvNotFinite; }
    if (used < 2) { *column = -1; return kConvFewSegments; }
    for (int j = 0; j < d; ++j)
        if (!(diag[j] > 0.0)) { *column = j; return kConvConstant; }
    *column = -1;
    return kConvOk;
}

// ---- the serial driver (host) ---------------------------------------------------------------------------------------------------
struct ConvResult {
    int status = 0, column = -1;
    int used = 0, skipped = 0;
    double r_minus_1 = NAN;
    std::vector<double> per_param;
};

// segs: (first row, rows) of row-major chains of ncols columns
inline void conv_serial(const std::vector<std::pair<const double*, int64_t>>& segs, int64_t ncols, int iw, int itheta, int d, ConvResult& out)
{
    out = ConvResult();
    const size_t S = segs.size();
    std::vector<double> W(S, 0.0), sum((size_t)d, 0.0), c((size_t)d, 0.0), a(S * d, 0.0);
    std::vector<int> bad_col((size_t)d, 0);
    bool bad_weight = false;
    double Wall = 0.0;
    for (size_t s = 0; s < S; ++s) {
        std::vector<double> part((size_t)d, 0.0);
        for (int64_t r = 0; r < segs[s].second; ++r) {
            const double* row = segs[s].first + r * ncols;
            const double w = row[iw];
            bad_weight = bad_weight || !conv_weight_ok(w);
            W[s] += w;
            for (int j = 0; j < d; ++j) {
                if (!conv_value_ok(row[itheta + j])) bad_col[(size_t)j] = 1;
                part[(size_t)j] += w * row[itheta + j];
            }
        }
        Wall += W[s];
        for (int j = 0; j < d; ++j) sum[(size_t)j] += part[(size_t)j];
    }
    std::vector<size_t> use;
    for (size_t s = 0; s < S; ++s)
        if (segs[s].second > 0 && W[s] > 0.0) use.push_back(s);
    out.used = (int)use.size();
    out.skipped = (int)(S - use.size());
    const int M = out.used;
    for (int j = 0; j < d; ++j) c[(size_t)j] = sum[(size_t)j] / Wall;
    std::vector<double> o((size_t)d, 0.0), diag((size_t)d, 0.0), Wc((size_t)d * d, 0.0);
    if (!bad_weight && M >= 2) {
        for (size_t s : use) {
            for (int64_t r = 0; r < segs[s].second; ++r) {
                const double* row = segs[s].first + r * ncols;
                for (int j = 0; j < d; ++j) a[s * d + j] += row[iw] * (row[itheta + j] - c[(size_t)j]);
            }
            for (int j = 0; j < d; ++j) {
                o[(size_t)j] += a[s * d + j];                      // W_s a_sj
                a[s * d + j] /= W[s];
            }
        }
        double Wu = 0.0;
        for (size_t s : use) Wu += W[s];
        for (int j = 0; j < d; ++j) o[(size_t)j] /= Wu;
        std::vector<double> y((size_t)d), Cs((size_t)d * d);
        for (size_t s : use) {
            std::fill(Cs.begin(), Cs.end(), 0.0);
            for (int64_t r = 0; r < segs[s].second; ++r) {
                const double* row = segs[s].first + r * ncols;
                for (int j = 0; j < d; ++j) y[(size_t)j] = (row[itheta + j] - c[(size_t)j]) - a[s * d + j];
                for (int i = 0; i < d; ++i) {
                    const double wy = row[iw] * y[(size_t)i];
                    for (int j = i; j < d; ++j) Cs[(size_t)i * d + j] = std::fma(wy, y[(size_t)j], Cs[(size_t)i * d + j]);
                }
            }
            for (int i = 0; i < d; ++i)
                for (int j = i; j < d; ++j) Wc[(size_t)i * d + j] += Cs[(size_t)i * d + j] / W[s];
        }
        for (int i = 0; i < d; ++i)
            for (int j = i; j < d; ++j) Wc[(size_t)j * d + i] = Wc[(size_t)i * d + j] = Wc[(size_t)i * d + j] / (double)M;
        for (int j = 0; j < d; ++j) diag[(size_t)j] = Wc[(size_t)j * d + j];
    }
    out.status = conv_status(bad_weight, bad_col.data(), M, diag.data(), d, &out.column);
    if (out.status != kConvOk) return;
    std::vector<double> sigma((size_t)d), dn((size_t)M * d), Wn((size_t)d * d);
    out.per_param.assign((size_t)d, 0.0);
    for (int j = 0; j < d; ++j) sigma[(size_t)j] = std::sqrt(diag[(size_t)j]);
    for (int k = 0; k < M; ++k)
        for (int j = 0; j < d; ++j) {
            const double delta = a[use[(size_t)k] * d + j] - o[(size_t)j];
            out.per_param[(size_t)j] += delta * delta;
            dn[(size_t)k * d + j] = delta / sigma[(size_t)j];
        }
    for (int j = 0; j < d; ++j) out.per_param[(size_t)j] = out.per_param[(size_t)j] / (double)(M - 1) / diag[(size_t)j];
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) Wn[(size_t)i * d + j] = i == j ? 1.0 : Wc[(size_t)i * d + j] / (sigma[(size_t)i] * sigma[(size_t)j]);
    std::vector<double> U((size_t)d * d), scale((size_t)d), lam((size_t)d), T((size_t)d * d, 0.0), v((size_t)d);
    int32_t stat[mce_eig::kStatInts];
    mce_eig::tournament_eig(Wn.data(), d, U.data(), scale.data(), lam.data(), stat);
    if (!conv_posdef(stat[mce_eig::kStatCode], lam[(size_t)d - 1], d)) {
        out.status = kConvNotPositive;
        out.column = stat[mce_eig::kStatIndex];
        return;
    }
    for (int k = 0; k < M; ++k) {
        for (int e = 0; e < d; ++e) {
            double t = 0.0;
            for (int j = 0; j < d; ++j) t = std::fma(U[(size_t)j * d + e], dn[(size_t)k * d + j], t);
            v[(size_t)e] = t * scale[(size_t)e];
        }
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) T[(size_t)i * d + j] = std::fma(v[(size_t)i], v[(size_t)j], T[(size_t)i * d + j]);
    }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) T[(size_t)i * d + j] = T[(size_t)i * d + j] / (double)(M - 1) + (i == j ? 1.0 : 0.0);
    mce_eig::tournament_eig(T.data(), d, U.data(), scale.data(), lam.data(), stat);
    out.r_minus_1 = lam[0] - 1.0;
}

}  // namespace mce_conv
