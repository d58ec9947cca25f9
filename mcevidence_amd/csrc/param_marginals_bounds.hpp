// param_marginals_bounds.hpp -- marginals= with bounds=: the 1-D marginal densities of param_marginals.hpp where a parameter has hard
// prior bounds (L, U): the grid ends on a bound it would cross, the density is Jones' linear boundary kernel in Jones & Foster's positive
// form, and the HPD sums give a grid that ends on a bound half a cell there.  Shared by the host check
// (tests/native/param_marginals_bounds_check.cpp, plain C++17 under g++) and the device kernels (param_marginals_kernels.hpp),
// as param_marginals.hpp is.  docs/design/marginals_bounds.md states the rule; mcevidence_amd/marginals.py (measure_bounded) restates
// it in NumPy.
//
// Steps 1 and 2 (the moments, h, c) are param_marginals.hpp's.  Per column with the bounds (L, U), -inf / +inf: that side is open:
//   3' a used value < L or > U: col_status 8, the column is NaN with pieces -1.  lo = min - 3 h; where L >= lo: lo = L, at_lo = 1.
//      hi = max + 3 h; where U <= hi: hi = U, at_hi = 1.  step and g_k as param_marginals.hpp forms them
//   4' over the used rows, in its row, tile and part order:  t = a_i K(c (g_k - x_i)^2),  S += t,  R += t (x_i - g_k) (a product, then a
//      sum);  T0 = S / norm,  T1 = (R / h) / norm,  norm = mar_norm(W, h)
//   5' p = (g - L) / h,  q = (U - g) / h,  phi(t) = t >= 40 ? 0 : exp(-t^2 / 2) / sqrt(2 pi),  psi(t) = t >= 40 ? 0 : t phi(t),
//      a0 = (erf(q / sqrt 2) + erf(p / sqrt 2)) / 2,  a1 = phi(p) - phi(q),  a2 = a0 - psi(q) - psi(p),  den = a0 a2 - a1 a1
//   6' f0 = T0 / a0,  f1 = (a2 T0 - a1 T1) / den,  rho = f0 > 0 ? f0 exp(min(f1 / f0, 4) - 1) : +0.0;  where den is not > 0 and
//      finite: rho = f0
//   7' the mode as in param_marginals.hpp
//   8' the HPD regions as in param_marginals.hpp, the order on rho, the running sum of w_k rho_k: w = 1/2 at k = 0 where at_lo, at
//      k = G - 1 where at_hi, 1 elsewhere
// A column without bounds is param_marginals.hpp's column bit for bit: a0 = 1, a1 = 0, a2 = 1, den = 1, f1 = f0 = T0, exp(0) = 1, w = 1,
// and S is summed in its order.
// Here:
//   * marb_bounds_ok, marb_params                                the bounds the rule takes; step 3' and the column's status;
//   * marb_term, marb_t0, marb_t1                                the pieces of step 4' as every route rounds them;
//   * marb_consts, marb_density                                  steps 5' and 6';
//   * marb_weighted                                              the end weights of step 8';
//   * the result block's layout (kMarb.., marb_out_doubles);
//   * mar_decide_ends, mar_serial_bounds                         the serial drivers of BOTH rules (mar_decide, mar_serial, marb_decide and
//                                                                marb_serial forward to them).
#pragma once

#include "param_marginals.hpp"

namespace mce_marb {

using namespace mce_mar;

enum : int { kMarbColOutside = 8 };
// the per-column rows after the head: param_marginals.hpp's, then these; the head's reserved slot holds 1
enum : int { kMarbBoundLo = kMarPerCol, kMarbBoundHi, kMarbAtLo, kMarbAtHi, kMarbPerCol };
static_assert(kMarbPerCol == 14, "the result block of include/mcevidence_hip.h");
constexpr double kMarbSqrt2 = 1.4142135623730951;              // sqrt(2), rounded to nearest
constexpr double kMarbFar = 40.0;                              // phi and psi are 0 from here on
constexpr double kMarbMaxSlope = 4.0;                          // the cap on f1 / f0

MCE_HD inline int64_t marb_out_doubles(int d, int np, int G) { return (int64_t)kMarHead + (int64_t)d * (kMarbPerCol + kMarPerP * np + G); }

// a pair of bounds the rule takes: neither is NaN, L < U (so L is not +inf and U is not -inf)
MCE_HD inline bool marb_bounds_ok(double L, double U) { return L < U; }

// steps 2 and 3' -> the column's status.  mn, mx: the smallest and the largest used value
MCE_HD inline int marb_params(double W, double A2, double v, double mn, double mx, double L, double U, double scale, int G, double* sd, double* h, double* c,
                              double* lo, double* step, double* at_lo, double* at_hi)
{
    MCE_MAR_NO_CONTRACT
    *at_lo = 0.0;
    *at_hi = 0.0;
    const int cs = mar_params(W, A2, v, mn, mx, scale, G, sd, h, c, lo, step);
    if (cs != kMarOk) return cs;
    if (mn < L || mx > U) return kMarbColOutside;
    const double m3 = 3.0 * *h;
    double hi = mx + m3;
    if (L >= *lo) { *lo = L; *at_lo = 1.0; }
    if (U <= hi) { hi = U; *at_hi = 1.0; }
    const double span = hi - *lo;
    *step = span / (double)(G - 1);
    return mar_pos_finite(*step) ? kMarOk : kMarColBad;
}

// one row's term of step 4': S + t and R + t (x - g), t = a K(c (g - x)^2); the argument as mar_arg rounds it, the sum S as mar_add does
MCE_HD inline void marb_term(double c, double g, double x, double a, double* S, double* R)
{
    MCE_MAR_NO_CONTRACT
    const double e = g - x;
    const double s = e * e;
    const double arg = c * s;
    if (arg >= mce_kde::kKdeUnderflow) return;                   // (t = +0.0: neither sum moves)
    const double t = a * exp(-arg);
    const double m = t * -e;
    *S = *S + t;
    *R = *R + m;
}
MCE_HD inline double marb_t0(double S, double norm) { return S / norm; }
MCE_HD inline double marb_t1(double R, double h, double norm)
{
    const double rh = R / h;
    return rh / norm;
}

MCE_HD inline double marb_phi(double t)
{
    MCE_MAR_NO_CONTRACT
    if (t >= kMarbFar) return 0.0;
    const double s = t * t;
    const double m = s / 2.0;
    return exp(-m) / kMarSqrt2Pi;
}
MCE_HD inline double marb_psi(double t)
{
    MCE_MAR_NO_CONTRACT
    if (t >= kMarbFar) return 0.0;
    return t * marb_phi(t);
}

// step 5' at the grid point g
MCE_HD inline void marb_consts(double g, double L, double U, double h, double* a0, double* a1, double* a2, double* den)
{
    MCE_MAR_NO_CONTRACT
    const double gl = g - L, ug = U - g;
    const double p = gl / h, q = ug / h;
    const double eq = erf(q / kMarbSqrt2), ep = erf(p / kMarbSqrt2);
    const double es = eq + ep;
    *a0 = 0.5 * es;
    *a1 = marb_phi(p) - marb_phi(q);
    const double d1 = *a0 - marb_psi(q);
    *a2 = d1 - marb_psi(p);
    const double m0 = *a0 * *a2, m1 = *a1 * *a1;
    *den = m0 - m1;
}

// step 6'
MCE_HD inline double marb_density(double T0, double T1, double a0, double a1, double a2, double den)
{
    MCE_MAR_NO_CONTRACT
    const double f0 = T0 / a0;
    if (!(f0 > 0.0)) return 0.0;
    if (!mar_pos_finite(den)) return f0;
    const double u = a2 * T0, v = a1 * T1;
    const double w = u - v;
    const double f1 = w / den;
    const double r = f1 / f0;
    const double rc = r < kMarbMaxSlope ? r : kMarbMaxSlope;
    const double ex = rc - 1.0;
    return f0 * exp(ex);
}

// w_k rho_k of step 8'
MCE_HD inline double marb_weighted(double rho, int k, int G, bool at_lo, bool at_hi)
{
    const bool half = (k == 0 && at_lo) || (k == G - 1 && at_hi);
    return half ? 0.5 * rho : rho;
}

}  // namespace mce_marb

// ---- the serial drivers (host): ONE text for param_marginals.hpp's rule and this one ----------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
namespace mce_mar {

// steps 5 and 6 (7' and 8') on the G densities of one column: mode[2] = the mode and its density; dec[p * kMarPerP ..]: lower, upper,
// pieces, edge.  at_lo / at_hi: the end weights of step 8' (neither: every weight is 1, and marb_weighted hands rho back as it is)
inline void mar_decide_ends(const double* rho, int G, double lo, double step, bool at_lo, bool at_hi, const double* probs, int np, double* mode, double* dec)
{
    std::vector<int> order((size_t)G);
    for (int k = 0; k < G; ++k) order[(size_t)k] = k;
    std::sort(order.begin(), order.end(), [rho](int a, int b) { return mar_before(rho[a], a, rho[b], b); });
    std::vector<double> cum((size_t)G);
    double run = 0.0;
    for (int p = 0; p < G; ++p) {
        run += mce_marb::marb_weighted(rho[order[(size_t)p]], order[(size_t)p], G, at_lo, at_hi);
        cum[(size_t)p] = run;
    }
    const double Z = run;
    mode[0] = mar_grid_point(lo, step, order[0]);
    mode[1] = rho[order[0]];
    std::vector<char> sel((size_t)G);
    for (int t = 0; t < np; ++t) {
        const double target = probs[t] * Z;
        int cut = G - 1;
        for (int p = 0; p < G; ++p)
            if (cum[(size_t)p] >= target) { cut = p; break; }
        std::fill(sel.begin(), sel.end(), 0);
        for (int p = 0; p <= cut; ++p) sel[(size_t)order[(size_t)p]] = 1;
        int kmin = G, kmax = -1, pieces = 0;
        for (int k = 0; k < G; ++k) {
            if (!sel[(size_t)k]) continue;
            kmin = k < kmin ? k : kmin;
            kmax = k;
            pieces += (k == 0 || !sel[(size_t)k - 1]) ? 1 : 0;
        }
        dec[t * kMarPerP + kMarLower] = mar_grid_point(lo, step, kmin);
        dec[t * kMarPerP + kMarUpper] = mar_grid_point(lo, step, kmax);
        dec[t * kMarPerP + kMarPieces] = (double)pieces;
        dec[t * kMarPerP + kMarEdge] = (sel[0] || sel[(size_t)G - 1]) ? 1.0 : 0.0;
    }
}

// the whole rule on one CPU thread.  bounds: null (param_marginals.hpp's rule, out: mar_out_doubles(d, np, G) doubles), or lo[d], then
// hi[d] (this file's, out: marb_out_doubles(d, np, G) doubles)
inline void mar_serial_bounds(const double* x, int64_t ld, int64_t n, int d, const double* w, const double* bounds, const double* probs, int np, int G, double scale,
                              double* out)
{
    using namespace mce_sum;
    using namespace mce_marb;
    const double nan = __builtin_nan("");
    const int per_col = bounds ? (int)kMarbPerCol : (int)kMarPerCol;
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
    const int status = mar_status(badw, badcol, W, rows, &column);
    mar_pack_head(status, column, W, A2, rows, G, np, out);
    if (bounds) out[kMarReserved] = 1.0;
    double* col = out + kMarHead;
    const int64_t total = (int64_t)d * (per_col + kMarPerP * np + G);
    for (int64_t k = 0; k < total; ++k) col[k] = nan;
    if (status != kMarOk) return;
    double* per_p = col + (int64_t)per_col * d;
    double* dens = per_p + (int64_t)kMarPerP * np * d;
    std::vector<double> dec((size_t)(kMarPerP * (np > 0 ? np : 1)));
    for (int j = 0; j < d; ++j) {
        const double L = bounds ? bounds[j] : nan, U = bounds ? bounds[d + j] : nan;
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
        double sd, h, c, lo, step, at_lo = 0.0, at_hi = 0.0;
        const int cs = bounds ? marb_params(W, A2, V / W, mn, mx, L, U, scale, G, &sd, &h, &c, &lo, &step, &at_lo, &at_hi)
                              : mar_params(W, A2, V / W, mn, mx, scale, G, &sd, &h, &c, &lo, &step);
        col[kMarColStatus * d + j] = (double)cs;
        if (bounds) {
            col[kMarbBoundLo * d + j] = L;
            col[kMarbBoundHi * d + j] = U;
        }
        if (cs != kMarOk) {
            for (int t = 0; t < np; ++t) per_p[(t * kMarPerP + kMarPieces) * d + j] = -1.0;
            continue;
        }
        col[kMarMean * d + j] = m;
        col[kMarVar * d + j] = V / W;
        col[kMarSd * d + j] = sd;
        col[kMarH * d + j] = h;
        col[kMarC * d + j] = c;
        col[kMarLo * d + j] = lo;
        col[kMarStep * d + j] = step;
        if (bounds) {
            col[kMarbAtLo * d + j] = at_lo;
            col[kMarbAtHi * d + j] = at_hi;
        }
        double* rho = dens + (int64_t)j * G;
        const double norm = mar_norm(W, h);
        for (int k = 0; k < G; ++k) {
            const double g = mar_grid_point(lo, step, k);
            if (!bounds) {
                double acc = 0.0;
                for (int64_t i : used) acc = mar_add(acc, w[i], mar_arg(c, g, x[i * ld + j]));
                rho[k] = acc / norm;
                continue;
            }
            double s0 = 0.0, s1 = 0.0;
            for (int64_t i : used) marb_term(c, g, x[i * ld + j], w[i], &s0, &s1);
            double a0, a1, a2, den;
            marb_consts(g, L, U, h, &a0, &a1, &a2, &den);
            rho[k] = marb_density(marb_t0(s0, norm), marb_t1(s1, h, norm), a0, a1, a2, den);
        }
        double mode[2];
        mar_decide_ends(rho, G, lo, step, at_lo != 0.0, at_hi != 0.0, probs, np, mode, dec.data());
        col[kMarMode * d + j] = mode[0];
        col[kMarModeDensity * d + j] = mode[1];
        for (int t = 0; t < np; ++t)
            for (int q = 0; q < kMarPerP; ++q) per_p[(t * kMarPerP + q) * d + j] = dec[(size_t)(t * kMarPerP + q)];
    }
}

}  // namespace mce_mar

namespace mce_marb {

// steps 7' and 8' on the G densities of one column
inline void marb_decide(const double* rho, int G, double lo, double step, bool at_lo, bool at_hi, const double* probs, int np, double* mode, double* dec)
{
    mar_decide_ends(rho, G, lo, step, at_lo, at_hi, probs, np, mode, dec);
}

// bounds: lo[d], then hi[d].  out: marb_out_doubles(d, np, G) doubles
inline void marb_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const double* bounds, const double* probs, int np, int G, double scale,
                        double* out)
{
    mar_serial_bounds(x, ld, n, d, w, bounds, probs, np, G, scale, out);
}

}  // namespace mce_marb
#endif
