// chain_corr.hpp -- the autocorrelation length of a chain and the thinning factor it gives (thin_corr), shared by the host check
// (tests/native/chain_corr_check.cpp, plain C++17 under g++) and the device kernels (chain_corr_kernels.hpp, __host__ __device__ under
// hipcc), after the pattern of chain_prep.hpp.  docs/design/chain_corr.md states the rule; mcevidence_amd/chains.py
// (correlation_length) restates it in NumPy.
//
// The SERIES of a part (one burned chain) is, under the integer rule, each row repeated trunc(w) times (weight units), under the bin
// rule the rows themselves (row units); the rule is mce_prep::choose_rule's verdict for thinlen = 2.  With U_p the units of part p
// and m_pj the mean of column j over part p's series:
//   S_j(t) = sum_p sum_{u < U_p - t} (y[p][u][j] - m_pj) (y[p][u + t][j] - m_pj)        (a pair never spans two parts)
//   n(t)   = sum_p max(U_p - t, 0),        rho_j(t) = (S_j(t) / n(t)) / (S_j(0) / n(0))
//   cap    = min(max_lag, max_p U_p / 4),  cut_j = the first t in 1 .. cap with rho_j(t) <= min_corr
//   L_j    = 1 + 2 sum_{t = 1}^{cut_j - 1} rho_j(t),    L = max_j L_j,    factor = max(1, ceil(scale L))
// Here:
//   * corr_cap               the cap;
//   * corr_unit_row          the row of unit u, from the inclusive int64 prefix sums of trunc(w) that mce_chain_weights_dev leaves;
//   * corr_mean              the centring value of a column of a part (a column that is constant over the part centres to exact zeros);
//   * corr_rho, CorrColumn / corr_advance, corr_length     cut and length of a column, fed one rho at a time in ascending lag;
//   * corr_status            ok / no cut within the cap / a constant column / a value that is not finite, with the column;
//   * corr_factor            the thinning factor;
//   * corr_serial            the serial driver: the whole rule on one CPU thread.
#pragma once

#include "chain_prep.hpp"

#include <utility>

namespace mce_corr {

enum : int {
    kCorrOk = 0,
    kCorrNoCut = 1,        // some column's rho stays above min_corr up to the cap
    kCorrConstant = 2,     // S_j(0) is not > 0
    kCorrNotFinite = 3     // a value of a measured column is NaN or infinite
};

constexpr double kCorrRuleThinlen = 2.0;      // the thinlen whose verdict (integer / bin / decline) fixes the units

MCE_HD inline int64_t corr_cap(int64_t max_lag, int64_t max_units)
{
    const int64_t q = max_units / 4;
    return max_lag < q ? max_lag : q;
}

// Unit u (0-based) of a part whose rows are first .. first + nrows - 1 of the concatenated numbering: the first row i of the part
// with c[first + i] - c_base >= u + 1, c the inclusive prefix sums over the concatenated rows and c_base = c[first - 1] (0 for
// first = 0).  0 <= u < the part's units.  Returns i (relative to the part); rows of weight 0 are never returned.
MCE_HD inline int64_t corr_unit_row(const int64_t* c, int64_t first, int64_t nrows, int64_t c_base, int64_t u)
{
    return mce_prep::int_lower_bound(c + first, nrows, c_base + u + 1);
}

// the centring value of a column of a part: sum / units, or the column's one value where it takes no other over the part
MCE_HD inline double corr_mean(double sum, double lo, double hi, int64_t units) { return lo == hi ? lo : sum / (double)units; }

MCE_HD inline double corr_rho(double s_tau, double n_tau, double s0, double n0) { return (s_tau / n_tau) / (s0 / n0); }

// cut and length of one column, advanced lag by lag from 1 upwards
struct CorrColumn {
    int64_t cut = 0;       // 0: not found yet
    double sum = 0.0;      // rho(1) + .. + rho(cut - 1), or up to the last lag seen
};
MCE_HD inline void corr_advance(CorrColumn& col, int64_t tau, double rho, double min_corr)
{
    if (col.cut != 0) return;
    if (rho <= min_corr) col.cut = tau;
    else col.sum += rho;
}
MCE_HD inline double corr_length(const CorrColumn& col) { return 1.0 + 2.0 * col.sum; }

// the status of a call from S_j(0) and the cuts (cut may be null before any lag was scanned): the first column that is not finite,
// else the first constant one, else the first without a cut
MCE_HD inline int corr_status(const double* s0, const int64_t* cut, int32_t ndim, int64_t* column)
{
    for (int32_t j = 0; j < ndim; ++j)
        if (!(s0[j] - s0[j] == 0.0)) { *column = j; return kCorrNotFinite; }
    for (int32_t j = 0; j < ndim; ++j)
        if (!(s0[j] > 0.0)) { *column = j; return kCorrConstant; }
    if (cut)
        for (int32_t j = 0; j < ndim; ++j)
            if (cut[j] == 0) { *column = j; return kCorrNoCut; }
    *column = -1;
    return kCorrOk;
}

inline int64_t corr_factor(double scale, double length)
{
    const double f = std::ceil(scale * length);
    return f > 1.0 ? (int64_t)f : 1;
}

// ---- the serial driver (host) ---------------------------------------------------------------------------------------------------
struct CorrResult {
    int rule = 0;              // mce_prep::kRuleInteger / kRuleBin, or the reason to decline (then nothing else is set)
    int status = 0;
    int64_t column = -1;       // the offending column of a non-zero status
    int64_t units = 0, max_units = 0, cap = 0, rho_rows = 0;
    std::vector<double> length, rho;      // L_j; rho[t * ndim + j] for t < rho_rows
    std::vector<int64_t> cut;
    double L = 0.0;
};

// parts: (first row, rows) of row-major chains of ncols columns
inline void corr_serial(const std::vector<std::pair<const double*, int64_t>>& parts, int64_t ncols, int iw, int itheta, int32_t ndim, double min_corr,
                        int64_t max_lag, CorrResult& out)
{
    out = CorrResult();
    std::vector<double> w;
    std::vector<int64_t> first;
    for (const auto& p : parts) {
        first.push_back((int64_t)w.size());
        for (int64_t i = 0; i < p.second; ++i) w.push_back(p.first[i * ncols + iw]);
    }
    const int64_t n = (int64_t)w.size();
    out.rule = mce_prep::choose_rule(kCorrRuleThinlen, mce_prep::weight_totals(w.data(), n));
    if (out.rule < 0) return;
    std::vector<int64_t> c((size_t)n);
    int64_t run = 0;
    for (int64_t i = 0; i < n; ++i) c[(size_t)i] = (run += mce_prep::weight_int(w[(size_t)i]));
    // the centred series of every part, unit-major
    std::vector<std::vector<double>> y(parts.size());
    std::vector<int64_t> units(parts.size());
    for (size_t p = 0; p < parts.size(); ++p) {
        const int64_t nr = parts[p].second, f = first[p];
        const int64_t base = f > 0 ? c[(size_t)f - 1] : 0;
        const int64_t U = nr == 0 ? 0 : (out.rule == mce_prep::kRuleInteger ? c[(size_t)(f + nr) - 1] - base : nr);
        units[p] = U;
        out.units += U;
        if (U > out.max_units) out.max_units = U;
        std::vector<int64_t> row((size_t)U);
        for (int64_t u = 0; u < U; ++u) row[(size_t)u] = out.rule == mce_prep::kRuleInteger ? corr_unit_row(c.data(), f, nr, base, u) : u;
        y[p].assign((size_t)(U * ndim), 0.0);
        for (int32_t j = 0; j < ndim; ++j) {
            double sum = 0.0, lo = INFINITY, hi = -INFINITY;
            for (int64_t u = 0; u < U; ++u) {
                const double v = parts[p].first[row[(size_t)u] * ncols + itheta + j];
                sum += v;
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
            const double m = corr_mean(sum, lo, hi, U);
            for (int64_t u = 0; u < U; ++u) y[p][(size_t)(u * ndim + j)] = parts[p].first[row[(size_t)u] * ncols + itheta + j] - m;
        }
    }
    out.cap = corr_cap(max_lag, out.max_units);
    std::vector<CorrColumn> cols((size_t)ndim);
    std::vector<double> s0((size_t)ndim, 0.0), s((size_t)ndim);
    double n0 = 0.0;
    for (int64_t tau = 0; tau <= out.cap; ++tau) {
        double nt = 0.0;
        for (int32_t j = 0; j < ndim; ++j) s[(size_t)j] = 0.0;
        for (size_t p = 0; p < parts.size(); ++p) {
            const int64_t U = units[p];
            if (U - tau <= 0) continue;
            nt += (double)(U - tau);
            for (int64_t u = 0; u + tau < U; ++u)
                for (int32_t j = 0; j < ndim; ++j) s[(size_t)j] += y[p][(size_t)(u * ndim + j)] * y[p][(size_t)((u + tau) * ndim + j)];
        }
        if (tau == 0) {
            s0 = s;
            n0 = nt;
            out.status = corr_status(s0.data(), nullptr, ndim, &out.column);
            if (out.status != kCorrOk) return;
        }
        bool all = tau > 0;
        for (int32_t j = 0; j < ndim; ++j) {
            const double rho = tau == 0 ? 1.0 : corr_rho(s[(size_t)j], nt, s0[(size_t)j], n0);
            out.rho.push_back(rho);
            if (tau > 0) corr_advance(cols[(size_t)j], tau, rho, min_corr);
            all = all && cols[(size_t)j].cut != 0;
        }
        out.rho_rows = tau + 1;
        if (all) break;
    }
    for (int32_t j = 0; j < ndim; ++j) {
        out.cut.push_back(cols[(size_t)j].cut);
        out.length.push_back(corr_length(cols[(size_t)j]));
        if (cols[(size_t)j].cut != 0 && out.length.back() > out.L) out.L = out.length.back();
    }
    out.status = corr_status(s0.data(), out.cut.data(), ndim, &out.column);
}

}  // namespace mce_corr
