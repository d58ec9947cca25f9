// param_contours.hpp -- the 2-D joint posterior densities behind contours= (a product-Gaussian kernel density estimate of every pair of
// chosen parameter columns on a regular G x G grid, its mode and its credible regions), shared by the host check
// (tests/native/param_contours_check.cpp, plain C++17 under g++) and the device kernels (param_contours_kernels.hpp,
// __host__ __device__ under hipcc), after the pattern of param_marginals.hpp.  docs/design/contours.md states the rule;
// mcevidence_amd/contours.py (measure) restates it in NumPy.
//
// A SYSTEM is one (x, ld, n, d, w) as in param_marginals.hpp; a row with a_r == 0 is skipped entirely.  cols[nc] is a strictly
// increasing list of chosen columns below d, 2 <= nc <= 32; the PAIRS are (cols[s], cols[t]), s < t, in the order (0,1), (0,2), ..,
// (nc-2, nc-1): P = nc (nc - 1) / 2 of them; the first column of a pair is its x axis.  All in fp64, G in {32, 64}, a bandwidth scale:
//   1  W, A2, m_j, v_j, min_j, max_j, ess, sd_j as param_marginals.hpp's step 1 (over all d columns: a value that is not finite in any
//      of them refuses the system, as there)
//   2  h_j = (scale * sd_j) * pow(1 / ess, 1 / 6),   c_j = 1 / ((2 * h_j) * h_j)     (the 2-D normal-reference rule at the Kish size)
//   3  lo_j = min_j - 3 * h_j,  hi_j = max_j + 3 * h_j,  step_j = (hi_j - lo_j) / (G - 1),  g_jk = mar_grid_point(lo_j, step_j, k)
//   4  E_j[r][k] = kde_kernel_arg_value(mar_arg(c_j, g_jk, x_rj)),   S_ij[kx][ky] = sum over used r of (a_r * E_i[r][kx]) * E_j[r][ky]
//      (the weight times the x axis' value is rounded, then multiplied by the y axis' value),
//      rho = S / (((W * h_i) * h_j) * (2 pi))
//   5  mode: the cell with the largest rho, the lowest flat index k = kx * G + ky among equals
//   6  for a probability p: the G * G cells ordered by rho descending, then k ascending; rho accumulated SERIALLY in that order, Z the
//      last running sum; selected = the positions up to and including the first whose running sum is >= p * Z (none: all); level = the
//      rho of the last selected position, cells = how many are selected, lower_x .. upper_y = the bounding box in grid points,
//      edge = 1 where a selected cell has kx or ky in {0, G - 1}
// The densities are DEFINED at the reported h, c, lo and step.  status of a system: param_marginals.hpp's 3, 5 and 6; with a status other
// than 0 every value is NaN.  col_status 7 by mar_params' condition on this rule's h, c, step; a pair with such a column has
// pair_status 7, NaN values and cells -1, and the other pairs do not notice.
//
// WITH HARD PRIOR BOUNDS (L_j, U_j) per chosen column, -inf / +inf: that side is open (docs/design/contours_bounds.md; contours.py's
// measure_bounded restates it).  Steps 1 and 2 as above; param_marginals_bounds.hpp's step 5' (marb_consts) and its cap on the slope:
//   3" a used value < L or > U: col_status 8 (7 comes first).  lo = min - 3 h; where L >= lo: lo = L, at_lo = 1.  hi = max + 3 h; where
//      U <= hi: hi = U, at_hi = 1.  step = (hi - lo) / (G - 1).  A pair with a failing column takes that column's status, the x axis' first
//   4" S as in step 4, bit for bit;  R_x = sum of ((a_r E_i) (x_ri - g_kx)) E_j,  R_y = sum of (a_r E_i) (E_j (x_rj - g_ky)): x - g is the
//      negated difference the argument was formed from; the first-moment sum of a column that is open on both sides is not formed and is
//      +0.0.  T00 = S / norm,  T10 = (R_x / h_i) / norm,  T01 = (R_y / h_j) / norm,  norm = con_norm(W, h_i, h_j)
//   5" u = (a0, a1, a2) and dx = den of the x axis at g_kx, v and dy of the y axis at g_ky, by marb_consts with this rule's h, lo, step
//   6" f0 = T00 / (u0 v0),  det = ((u0 v0) dx) dy,
//      f1 = ((T00 ((u0 u2) (v0 v2) - (u1 u1) (v1 v1)) - T10 ((u0 u1) dy)) - T01 ((v0 v1) dx)) / det,
//      rho = f0 > 0 ? f0 exp(min(f1 / f0, 4) - 1) : +0.0;  where det is not > 0 and finite: rho = f0     (conb_density has the order)
//   7" the mode as in step 5
//   8" step 6 on rho, the running sum of (w_kx w_ky) rho: w = 1/2 at k = 0 where at_lo, at k = G - 1 where at_hi, 1 elsewhere; the
//      weight (1, 1/2 or 1/4) is formed first
// A pair whose two columns are open is the pair of the rule above bit for bit: u = v = (1, 0, 1), dx = dy = 1, f1 = f0 = T00, exp(0) = 1,
// w = 1, and S is summed in its order.  The result block has the column rows bound_lo, bound_hi, at_lo, at_hi after col_status.
#pragma once

#include <stdint.h>

#include <cmath>

#include "kde_shift.hpp"
#include "param_marginals.hpp"
#include "param_marginals_bounds.hpp"
#include "param_summary.hpp"
#include "seg_tiles.hpp"

#ifndef MCE_CONTOURS_HEAD
#define MCE_CONTOURS_HEAD 8
#endif
#ifndef MCE_CONTOURS_MAX_COLS
#define MCE_CONTOURS_MAX_COLS 32
#endif

namespace mce_con {

enum : int { kConOk = 0, kConColBad = mce_mar::kMarColBad };
// the head of a result block
enum : int { kConW = 0, kConA2, kConRows, kConStatus, kConColumn, kConGrid, kConNp, kConNc, kConHead };
static_assert(kConHead == MCE_CONTOURS_HEAD, "the result block of include/mcevidence_hip.h");
// after the head: kConPerCol rows of nc; kConPerPair rows of P; per probability kConPerP rows of P; then density[P][G][G]
enum : int { kConCol = 0, kConMean, kConVar, kConSd, kConH, kConC, kConLo, kConStep, kConColStatus, kConPerCol };
enum : int { kConModeX = 0, kConModeY, kConModeDensity, kConPairStatus, kConPerPair };
enum : int { kConLevel = 0, kConCells, kConLowerX, kConUpperX, kConLowerY, kConUpperY, kConEdge, kConPerP };
constexpr int kConMaxCols = MCE_CONTOURS_MAX_COLS;
constexpr int kConMaxPairs = kConMaxCols * (kConMaxCols - 1) / 2;
constexpr int kConMaxP = mce_mar::kMarMaxP;
constexpr int kConMaxGrid = 64;
constexpr int kConMaxParts = 16;                                // parts of a system's rows
constexpr int kConBlock = 256;                                  // cells of a fold workgroup
constexpr double kConTwoPi = 6.283185307179586;                 // 2 pi, rounded to nearest

MCE_HD inline bool con_grid_ok(int G) { return G == 32 || G == 64; }
MCE_HD inline bool con_nc_ok(int nc) { return nc >= 2 && nc <= kConMaxCols; }
MCE_HD inline int con_npairs(int nc) { return nc * (nc - 1) / 2; }
MCE_HD inline int64_t con_out_doubles(int nc, int np, int G)
{
    return (int64_t)kConHead + (int64_t)kConPerCol * nc + (int64_t)con_npairs(nc) * (kConPerPair + kConPerP * np + G * G);
}
// the pair (s, t), s < t < nc, in the order (0,1), (0,2), .., (nc-2, nc-1)
MCE_HD inline int con_pair_index(int s, int t, int nc) { return s * (2 * nc - s - 1) / 2 + (t - s - 1); }
MCE_HD inline int con_nparts(int64_t n)
{
    const int64_t t = mce_seg::seg_ntiles(n);
    return t < kConMaxParts ? (int)t : kConMaxParts;
}
// the first tile of part p (p = nparts: the end): mar_part_tile's formula
MCE_HD inline int64_t con_part_tile(int64_t n, int p)
{
    const int np = con_nparts(n);
    return np > 0 ? mce_seg::seg_ntiles(n) * p / np : 0;
}

// steps 2 and 3 -> the column's status
MCE_HD inline int con_params(double W, double A2, double v, double mn, double mx, double scale, int G, double* sd, double* h, double* c, double* lo, double* step)
{
    MCE_MAR_NO_CONTRACT
    const double ess = W * W / A2;
    *sd = sqrt(v);
    const double t = 1.0 / ess;
    const double f = pow(t, 1.0 / 6.0);
    const double sc = scale * *sd;
    *h = sc * f;
    const double h2 = 2.0 * *h;
    *c = 1.0 / (h2 * *h);
    const double m3 = 3.0 * *h;
    *lo = mn - m3;
    const double hi = mx + m3;
    const double span = hi - *lo;
    *step = span / (double)(G - 1);
    const bool ok = *sd > 0.0 && mce_mar::mar_pos_finite(*h) && mce_mar::mar_pos_finite(*c) && mce_mar::mar_pos_finite(*step);
    return ok ? kConOk : kConColBad;
}

// one kernel value E_j[r][k]
MCE_HD inline double con_value(double c, double g, double x) { return mce_kde::kde_kernel_arg_value(mce_mar::mar_arg(c, g, x)); }
// a_r * E_i[r][kx]: rounded once
MCE_HD inline double con_weighted(double a, double e) { return a * e; }
// S + ae * E_j[r][ky]
MCE_HD inline double con_add(double S, double ae, double ey)
{
    MCE_MAR_NO_CONTRACT
    const double t = ae * ey;
    return S + t;
}
MCE_HD inline double con_norm(double W, double hx, double hy)
{
    MCE_MAR_NO_CONTRACT
    const double wh = W * hx;
    const double whh = wh * hy;
    return whh * kConTwoPi;
}

// ---- with hard prior bounds ------------------------------------------------------------------------------------------------------------
enum : int { kConbColOutside = mce_marb::kMarbColOutside };
// the per-column rows after the head: the rule's above, then these
enum : int { kConbBoundLo = kConPerCol, kConbBoundHi, kConbAtLo, kConbAtHi, kConbPerCol };
static_assert(kConbPerCol == 13, "the result block of include/mcevidence_hip.h");
MCE_HD inline int64_t conb_out_doubles(int nc, int np, int G)
{
    return (int64_t)kConHead + (int64_t)kConbPerCol * nc + (int64_t)con_npairs(nc) * (kConPerPair + kConPerP * np + G * G);
}
// is the column open on both sides?  (its first-moment sum is not formed)
MCE_HD inline bool conb_open(double L, double U) { return L == -HUGE_VAL && U == HUGE_VAL; }

// steps 2 and 3" -> the column's status
MCE_HD inline int conb_params(double W, double A2, double v, double mn, double mx, double L, double U, double scale, int G, double* sd, double* h, double* c,
                              double* lo, double* step, double* at_lo, double* at_hi)
{
    MCE_MAR_NO_CONTRACT
    *at_lo = 0.0;
    *at_hi = 0.0;
    const int cs = con_params(W, A2, v, mn, mx, scale, G, sd, h, c, lo, step);
    if (cs != kConOk) return cs;
    if (mn < L || mx > U) return kConbColOutside;
    const double m3 = 3.0 * *h;
    double hi = mx + m3;
    if (L >= *lo) { *lo = L; *at_lo = 1.0; }
    if (U <= hi) { hi = U; *at_hi = 1.0; }
    const double span = hi - *lo;
    *step = span / (double)(G - 1);
    return mce_mar::mar_pos_finite(*step) ? kConOk : kConColBad;
}
// the status of a pair from its columns': the x axis' first
MCE_HD inline int conb_pair_status(int cs, int ct) { return cs != kConOk ? cs : ct; }

// x - g: the negated difference mar_arg forms the argument from
MCE_HD inline double conb_moment_arm(double g, double x)
{
    const double e = g - x;
    return -e;
}
// (a E_i) (x_i - g) of the x axis, E_j (x_j - g) of the y axis: one product
MCE_HD inline double conb_moment(double e, double arm) { return e * arm; }
MCE_HD inline double conb_t1(double R, double h, double norm)
{
    const double rh = R / h;
    return rh / norm;
}

// step 6": u[4], v[4] = a0, a1, a2, den of the x and the y axis
MCE_HD inline double conb_density(double T00, double T10, double T01, const double* u, const double* v)
{
    MCE_MAR_NO_CONTRACT
    const double uv0 = u[0] * v[0];
    const double f0 = T00 / uv0;
    if (!(f0 > 0.0)) return 0.0;
    const double d1 = uv0 * u[3];
    const double det = d1 * v[3];
    if (!mce_mar::mar_pos_finite(det)) return f0;
    const double u02 = u[0] * u[2], v02 = v[0] * v[2], u11 = u[1] * u[1], v11 = v[1] * v[1];
    const double m1 = u02 * v02, m2 = u11 * v11;
    const double k00 = m1 - m2;
    const double u01 = u[0] * u[1], v01 = v[0] * v[1];
    const double k10 = u01 * v[3], k01 = v01 * u[3];
    const double w0 = T00 * k00, w1 = T10 * k10, w2 = T01 * k01;
    const double w01 = w0 - w1;
    const double w = w01 - w2;
    const double f1 = w / det;
    const double r = f1 / f0;
    const double rc = r < mce_marb::kMarbMaxSlope ? r : mce_marb::kMarbMaxSlope;
    const double ex = rc - 1.0;
    return f0 * exp(ex);
}

// (w_kx w_ky) rho of step 8", k = kx * G + ky
MCE_HD inline double conb_weighted(double rho, int k, int G, bool x_lo, bool x_hi, bool y_lo, bool y_hi)
{
    const int kx = k / G, ky = k % G;
    const double wx = ((kx == 0 && x_lo) || (kx == G - 1 && x_hi)) ? 0.5 : 1.0;
    const double wy = ((ky == 0 && y_lo) || (ky == G - 1 && y_hi)) ? 0.5 : 1.0;
    const double w = wx * wy;
    return w * rho;
}

MCE_HD inline void con_pack_head(int status, int column, double W, double A2, double rows, int G, int np, int nc, double* out)
{
    const bool ok = status == mce_mar::kMarOk;
    const double nan = __builtin_nan("");
    out[kConW] = ok ? W : nan;
    out[kConA2] = ok ? A2 : nan;
    out[kConRows] = rows;
    out[kConStatus] = (double)status;
    out[kConColumn] = (double)column;
    out[kConGrid] = (double)G;
    out[kConNp] = (double)np;
    out[kConNc] = (double)nc;
}

}  // namespace mce_con

// ---- the serial drivers (host) --------------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>

namespace mce_con {

// steps 5 and 6 (7" and 8") on the G * G densities of one pair: mode[3] = mode_x, mode_y and its density; dec[p * kConPerP ..].
// ends[4] = at_lo, at_hi of the x axis, then of the y axis: the end weights of step 8" (none: every weight is 1)
inline void con_decide_ends(const double* rho, int G, double lox, double stepx, double loy, double stepy, const bool* ends, const double* probs, int np, double* mode,
                            double* dec)
{
    const int N = G * G;
    std::vector<int> order((size_t)N);
    for (int k = 0; k < N; ++k) order[(size_t)k] = k;
    std::sort(order.begin(), order.end(), [rho](int a, int b) { return mce_mar::mar_before(rho[a], a, rho[b], b); });
    std::vector<double> cum((size_t)N);
    double run = 0.0;
    for (int p = 0; p < N; ++p) {
        run += conb_weighted(rho[order[(size_t)p]], order[(size_t)p], G, ends[0], ends[1], ends[2], ends[3]);
        cum[(size_t)p] = run;
    }
    const double Z = run;
    mode[0] = mce_mar::mar_grid_point(lox, stepx, order[0] / G);
    mode[1] = mce_mar::mar_grid_point(loy, stepy, order[0] % G);
    mode[2] = rho[order[0]];
    for (int t = 0; t < np; ++t) {
        const double target = probs[t] * Z;
        int cut = N - 1;
        for (int p = 0; p < N; ++p)
            if (cum[(size_t)p] >= target) { cut = p; break; }
        int x0 = G, x1 = -1, y0 = G, y1 = -1, edge = 0;
        for (int p = 0; p <= cut; ++p) {
            const int kx = order[(size_t)p] / G, ky = order[(size_t)p] % G;
            x0 = kx < x0 ? kx : x0;
            x1 = kx > x1 ? kx : x1;
            y0 = ky < y0 ? ky : y0;
            y1 = ky > y1 ? ky : y1;
            edge |= (kx == 0 || kx == G - 1 || ky == 0 || ky == G - 1) ? 1 : 0;
        }
        double* o = dec + t * kConPerP;
        o[kConLevel] = rho[order[(size_t)cut]];
        o[kConCells] = (double)(cut + 1);
        o[kConLowerX] = mce_mar::mar_grid_point(lox, stepx, x0);
        o[kConUpperX] = mce_mar::mar_grid_point(lox, stepx, x1);
        o[kConLowerY] = mce_mar::mar_grid_point(loy, stepy, y0);
        o[kConUpperY] = mce_mar::mar_grid_point(loy, stepy, y1);
        o[kConEdge] = (double)edge;
    }
}
inline void con_decide(const double* rho, int G, double lox, double stepx, double loy, double stepy, const double* probs, int np, double* mode, double* dec)
{
    const bool ends[4] = {false, false, false, false};
    con_decide_ends(rho, G, lox, stepx, loy, stepy, ends, probs, np, mode, dec);
}

// the whole rule on one CPU thread.  bounds: null (the rule without bounds, out: con_out_doubles(nc, np, G) doubles), or lo[nc], then
// hi[nc] of the chosen columns (out: conb_out_doubles(nc, np, G) doubles)
inline void con_serial_bounds(const double* x, int64_t ld, int64_t n, int d, const double* w, const int32_t* cols, int nc, const double* bounds, const double* probs,
                              int np, int G, double scale, double* out)
{
    using namespace mce_sum;
    const double nan = __builtin_nan("");
    const int per_col = bounds ? (int)kConbPerCol : (int)kConPerCol;
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
    const int status = mce_mar::mar_status(badw, badcol, W, rows, &column);
    con_pack_head(status, column, W, A2, rows, G, np, nc, out);
    const int P = con_npairs(nc), N = G * G;
    const int64_t total = (bounds ? conb_out_doubles(nc, np, G) : con_out_doubles(nc, np, G)) - kConHead;
    double* col = out + kConHead;
    for (int64_t k = 0; k < total; ++k) col[k] = nan;
    for (int t = 0; t < nc; ++t) col[kConCol * nc + t] = (double)cols[t];
    if (status != mce_mar::kMarOk) return;
    double* pair = col + (int64_t)per_col * nc;
    double* per_p = pair + (int64_t)kConPerPair * P;
    double* dens = per_p + (int64_t)kConPerP * np * P;
    std::vector<double> h((size_t)nc), c((size_t)nc), lo((size_t)nc), step((size_t)nc), L((size_t)nc, -HUGE_VAL), U((size_t)nc, HUGE_VAL);
    std::vector<double> at_lo((size_t)nc, 0.0), at_hi((size_t)nc, 0.0), tab((size_t)nc * (size_t)G * 4);
    std::vector<int> cs((size_t)nc);
    for (int t = 0; t < nc; ++t) {
        const int j = cols[t];
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
        double sd;
        if (bounds) {
            L[(size_t)t] = bounds[t];
            U[(size_t)t] = bounds[nc + t];
            cs[(size_t)t] = conb_params(W, A2, V / W, mn, mx, L[(size_t)t], U[(size_t)t], scale, G, &sd, &h[(size_t)t], &c[(size_t)t], &lo[(size_t)t], &step[(size_t)t],
                                        &at_lo[(size_t)t], &at_hi[(size_t)t]);
            col[kConbBoundLo * nc + t] = L[(size_t)t];
            col[kConbBoundHi * nc + t] = U[(size_t)t];
        } else {
            cs[(size_t)t] = con_params(W, A2, V / W, mn, mx, scale, G, &sd, &h[(size_t)t], &c[(size_t)t], &lo[(size_t)t], &step[(size_t)t]);
        }
        col[kConColStatus * nc + t] = (double)cs[(size_t)t];
        if (cs[(size_t)t] != kConOk) continue;
        col[kConMean * nc + t] = m;
        col[kConVar * nc + t] = V / W;
        col[kConSd * nc + t] = sd;
        col[kConH * nc + t] = h[(size_t)t];
        col[kConC * nc + t] = c[(size_t)t];
        col[kConLo * nc + t] = lo[(size_t)t];
        col[kConStep * nc + t] = step[(size_t)t];
        if (bounds) {
            col[kConbAtLo * nc + t] = at_lo[(size_t)t];
            col[kConbAtHi * nc + t] = at_hi[(size_t)t];
            for (int k = 0; k < G; ++k) {
                double* q = &tab[((size_t)t * (size_t)G + (size_t)k) * 4];
                mce_marb::marb_consts(mce_mar::mar_grid_point(lo[(size_t)t], step[(size_t)t], k), L[(size_t)t], U[(size_t)t], h[(size_t)t], q, q + 1, q + 2, q + 3);
            }
        }
    }
    // ex: a_r E_s[r][kx];  ey: E_t[r][ky];  mx, my: the same times x - g, formed for a column that is not open
    std::vector<double> ex(used.size() * (size_t)G), ey(used.size() * (size_t)G), mxv, myv, dec((size_t)(kConPerP * (np > 0 ? np : 1)));
    if (bounds) {
        mxv.resize(ex.size());
        myv.resize(ey.size());
    }
    for (int s = 0; s < nc; ++s) {
        const bool sx = bounds && !conb_open(L[(size_t)s], U[(size_t)s]);
        if (cs[(size_t)s] == kConOk)
            for (size_t q = 0; q < used.size(); ++q)
                for (int k = 0; k < G; ++k) {
                    const double g = mce_mar::mar_grid_point(lo[(size_t)s], step[(size_t)s], k), xv = x[used[q] * ld + cols[s]];
                    ex[q * G + k] = con_weighted(w[used[q]], con_value(c[(size_t)s], g, xv));
                    if (sx) mxv[q * G + k] = conb_moment(ex[q * G + k], conb_moment_arm(g, xv));
                }
        for (int t = s + 1; t < nc; ++t) {
            const int p = con_pair_index(s, t, nc);
            const int ps = conb_pair_status(cs[(size_t)s], cs[(size_t)t]);
            pair[kConPairStatus * P + p] = (double)ps;
            if (ps != kConOk) {
                for (int q = 0; q < np; ++q) per_p[(q * kConPerP + kConCells) * P + p] = -1.0;
                continue;
            }
            const bool sy = bounds && !conb_open(L[(size_t)t], U[(size_t)t]);
            for (size_t q = 0; q < used.size(); ++q)
                for (int k = 0; k < G; ++k) {
                    const double g = mce_mar::mar_grid_point(lo[(size_t)t], step[(size_t)t], k), xv = x[used[q] * ld + cols[t]];
                    ey[q * G + k] = con_value(c[(size_t)t], g, xv);
                    if (sy) myv[q * G + k] = conb_moment(ey[q * G + k], conb_moment_arm(g, xv));
                }
            double* rho = dens + (int64_t)p * N;
            const double norm = con_norm(W, h[(size_t)s], h[(size_t)t]);
            for (int kx = 0; kx < G; ++kx)
                for (int ky = 0; ky < G; ++ky) {
                    double acc = 0.0, rx = 0.0, ry = 0.0;
                    for (size_t q = 0; q < used.size(); ++q) acc = con_add(acc, ex[q * G + kx], ey[q * G + ky]);
                    if (!bounds) {
                        rho[kx * G + ky] = acc / norm;
                        continue;
                    }
                    if (sx)
                        for (size_t q = 0; q < used.size(); ++q) rx = con_add(rx, mxv[q * G + kx], ey[q * G + ky]);
                    if (sy)
                        for (size_t q = 0; q < used.size(); ++q) ry = con_add(ry, ex[q * G + kx], myv[q * G + ky]);
                    rho[kx * G + ky] = conb_density(acc / norm, conb_t1(rx, h[(size_t)s], norm), conb_t1(ry, h[(size_t)t], norm), &tab[((size_t)s * (size_t)G + (size_t)kx) * 4],
                                                    &tab[((size_t)t * (size_t)G + (size_t)ky) * 4]);
                }
            double mode[3];
            const bool ends[4] = {at_lo[(size_t)s] != 0.0, at_hi[(size_t)s] != 0.0, at_lo[(size_t)t] != 0.0, at_hi[(size_t)t] != 0.0};
            con_decide_ends(rho, G, lo[(size_t)s], step[(size_t)s], lo[(size_t)t], step[(size_t)t], ends, probs, np, mode, dec.data());
            pair[kConModeX * P + p] = mode[0];
            pair[kConModeY * P + p] = mode[1];
            pair[kConModeDensity * P + p] = mode[2];
            for (int q = 0; q < np; ++q)
                for (int z = 0; z < kConPerP; ++z) per_p[(q * kConPerP + z) * P + p] = dec[(size_t)(q * kConPerP + z)];
        }
    }
}

// out: con_out_doubles(nc, np, G) doubles
inline void con_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const int32_t* cols, int nc, const double* probs, int np, int G, double scale,
                       double* out)
{
    con_serial_bounds(x, ld, n, d, w, cols, nc, nullptr, probs, np, G, scale, out);
}
// bounds: lo[nc], then hi[nc].  out: conb_out_doubles(nc, np, G) doubles
inline void conb_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const int32_t* cols, int nc, const double* bounds, const double* probs, int np,
                        int G, double scale, double* out)
{
    con_serial_bounds(x, ld, n, d, w, cols, nc, bounds, probs, np, G, scale, out);
}

}  // namespace mce_con
#endif
