// chain_prep.hpp -- what happens to a chain between "parsed" and "fed": burn-in and the thinning rules, shared by the host check
// (tests/native/chain_prep_check.cpp, plain C++17 under g++) and the device kernels (chain_prep_kernels.hpp, __host__ __device__
// under hipcc), after the pattern of chain_parse.hpp.
//
// The rules are those of mcevidence_amd/chains.py (removeBurn, integer_weight_thin, max_weight_bin_thin), which
// tests/golden/host_pins.json pins; here they are restated per element, so that a kernel can apply one of them to one row:
//   * burn_start            the first row a chain keeps;
//   * weight_ok / weight_int / weight_frac     what a weight contributes to the decision "integer weights or not";
//   * choose_rule           none / integer / bin, or a reason to decline, from the totals over all weights;
//   * int_keep_flag         integer rule, factor >= max weight: keep row i iff it is the first or c[i] / f != c[i-1] / f,
//                           c the inclusive prefix sum of the truncated weights;
//   * int_lower_bound       integer rule, factor < max weight: output m (1-based) is the first row with c[i] >= m f;
//   * bin_range / bin_better      bin rule: the rows of bin b (the host's np.digitize against edges computed ON THE HOST by
//                           np.linspace, so that no kernel re-derives a rounded edge) and "first row of maximal weight".
// thin_select is the serial driver: the same rules applied to a whole weight vector on one CPU thread.
#pragma once

#include <stdint.h>

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

#include <cmath>
#include <vector>

namespace mce_prep {

enum : int {
    kRuleNone = 0,       // thinlen 0 or 1: every row, weights untouched
    kRuleInteger = 1,    // integer_weight_thin
    kRuleBin = 2,        // max_weight_bin_thin
    // reasons to decline (the caller runs the host route, which words its own errors)
    kDeclineBadWeight = -1,    // a weight is negative, not finite or beyond 2^53
    kDeclineAmbiguous = -2,    // the sum of the fractional parts lies within kAmbiguousBand of kIntegerSumTol
    kDeclineThinlen = -3       // thinlen < 0 (the host raises) or 0 < thinlen < 1 (Poisson draws from the host's RNG)
};

constexpr double kIntegerSumTol = 1e-4;      // chains.py: abs(sum(trunc(w)) - sum(w)) > 1e-4 -> not integer weights
constexpr double kAmbiguousBand = 1e-6;      // the host forms that difference from two rounded sums: no guessing this near the threshold
constexpr double kMaxWeight = 9007199254740992.0;      // 2^53: beyond it w - trunc(w) says nothing and trunc(w) may not fit

// totals over the burned, concatenated weight column
struct WeightTotals {
    int64_t sum_int = 0;     // sum of trunc(w), exact
    int64_t max_int = 0;     // max of trunc(w)
    double frac = 0.0;       // sum of w - trunc(w), each term exact, added in a fixed order
    int64_t bad = 0;         // weights for which weight_ok is false
};

// removeBurn: burn < 1 is a fraction of the chain, otherwise a row count; burn <= 0 keeps everything (chains2samples burns only
// when burnlen > 0); a start at or beyond the end leaves an empty chain
MCE_HD inline int64_t burn_start(int64_t nrows, double burn)
{
    if (!(burn > 0.0)) return 0;
    const double s = burn < 1.0 ? (double)nrows * burn : burn;
    if (s >= (double)nrows) return nrows;
    return (int64_t)s;
}

MCE_HD inline bool weight_ok(double w) { return w >= 0.0 && w <= kMaxWeight; }      // (false for NaN)
MCE_HD inline int64_t weight_int(double w) { return weight_ok(w) ? (int64_t)w : 0; }
MCE_HD inline double weight_frac(double w) { return weight_ok(w) ? w - (double)(int64_t)w : 0.0; }

MCE_HD inline int choose_rule(double thinlen, const WeightTotals& t)
{
    if (thinlen == 0.0 || thinlen == 1.0) return kRuleNone;
    if (!(thinlen > 1.0)) return kDeclineThinlen;
    if (t.bad > 0) return kDeclineBadWeight;
    if (thinlen != std::floor(thinlen) || thinlen > kMaxWeight) return kRuleBin;
    if (std::fabs(t.frac - kIntegerSumTol) < kAmbiguousBand) return kDeclineAmbiguous;
    return t.frac <= kIntegerSumTol ? kRuleInteger : kRuleBin;
}

// integer rule, first branch (factor >= max weight).  c_prev is ignored for the first row.
MCE_HD inline bool int_keep_flag(int64_t c_prev, int64_t c, int64_t factor, bool first) { return first || c / factor != c_prev / factor; }

// integer rule, second branch: the first i in [0, n) with c[i] >= target (c never decreases; target <= c[n-1])
MCE_HD inline int64_t int_lower_bound(const int64_t* c, int64_t n, int64_t target)
{
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (c[mid] >= target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// bin rule: row i belongs to bin #{edges <= i} (np.digitize), so bin b (1-based, 1 .. nedges) holds the rows
// ceil(edges[b-1]) <= i < ceil(edges[b]) (no upper edge for b = nedges), cut to [0, n)
MCE_HD inline void bin_range(const double* edges, int64_t nedges, int64_t b, int64_t n, int64_t* lo, int64_t* hi)
{
    const double a = std::ceil(edges[b - 1]);
    int64_t l = a <= 0.0 ? 0 : (a >= (double)n ? n : (int64_t)a), h = n;
    if (b < nedges) {
        const double z = std::ceil(edges[b]);
        h = z <= 0.0 ? 0 : (z >= (double)n ? n : (int64_t)z);
    }
    if (h < l) h = l;
    *lo = l;
    *hi = h;
}
// is row i (weight w) a better representative of its bin than row bi (weight bw; bi < 0: none yet)?
MCE_HD inline bool bin_better(double w, int64_t i, double bw, int64_t bi) { return bi < 0 || w > bw || (w == bw && i < bi); }

// ---- the serial driver (host) ---------------------------------------------------------------------------------------------------
inline WeightTotals weight_totals(const double* w, int64_t n)
{
    WeightTotals t;
    for (int64_t i = 0; i < n; ++i) {
        if (!weight_ok(w[i])) { ++t.bad; continue; }
        const int64_t wi = weight_int(w[i]);
        t.sum_int += wi;
        if (wi > t.max_int) t.max_int = wi;
        t.frac += weight_frac(w[i]);
    }
    return t;
}

// keep / new_w for `thinlen` over w[0..n), edges[nedges] as np.linspace(-1, n, nbins + 1) gives them (read by the bin rule only).
// Returns the rule taken or the reason to decline (then keep / new_w are empty).  force_rule: kRuleInteger / kRuleBin apply that rule
// whatever choose_rule says (the bin rule with a unit below 1 is reachable through chains.max_weight_bin_thin only).
inline int thin_select(const double* w, int64_t n, double thinlen, const double* edges, int64_t nedges, std::vector<int64_t>& keep,
                       std::vector<double>& new_w, int force_rule = kRuleNone)
{
    keep.clear();
    new_w.clear();
    const WeightTotals t = weight_totals(w, n);
    const int rule = force_rule != kRuleNone ? force_rule : choose_rule(thinlen, t);
    if (rule == kRuleNone) {
        for (int64_t i = 0; i < n; ++i) { keep.push_back(i); new_w.push_back(w[i]); }
    } else if (rule == kRuleInteger) {
        const int64_t factor = (int64_t)thinlen;
        std::vector<int64_t> c((size_t)n);
        int64_t run = 0;
        for (int64_t i = 0; i < n; ++i) c[(size_t)i] = (run += weight_int(w[i]));
        if (factor >= t.max_int) {
            for (int64_t i = 0; i < n; ++i)
                if (int_keep_flag(i ? c[(size_t)i - 1] : 0, c[(size_t)i], factor, i == 0)) keep.push_back(i);
        } else {
            const int64_t nout = n > 0 ? c[(size_t)n - 1] / factor : 0;
            for (int64_t m = 1; m <= nout; ++m) keep.push_back(int_lower_bound(c.data(), n, m * factor));
        }
        for (int64_t i : keep) new_w.push_back((double)weight_int(w[i]));
    } else if (rule == kRuleBin) {
        for (int64_t b = 1; b <= nedges; ++b) {
            int64_t lo, hi, best = -1;
            bin_range(edges, nedges, b, n, &lo, &hi);
            for (int64_t i = lo; i < hi; ++i)
                if (bin_better(w[i], i, best < 0 ? 0.0 : w[best], best)) best = i;
            if (best >= 0) { keep.push_back(best); new_w.push_back(w[best]); }
        }
    }
    return rule;
}

}  // namespace mce_prep
