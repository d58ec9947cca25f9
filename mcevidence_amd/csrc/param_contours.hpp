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
#pragma once

#include <stdint.h>

#include <cmath>

#include "kde_shift.hpp"
#include "param_marginals.hpp"
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

// steps 5 and 6 on the G * G densities of one pair: mode[3] = mode_x, mode_y and its density; dec[p * kConPerP ..]
inline void con_decide(const double* rho, int G, double lox, double stepx, double loy, double stepy, const double* probs, int np, double* mode, double* dec)
{
    const int N = G * G;
    std::vector<int> order((size_t)N);
    for (int k = 0; k < N; ++k) order[(size_t)k] = k;
    std::sort(order.begin(), order.end(), [rho](int a, int b) { return mce_mar::mar_before(rho[a], a, rho[b], b); });
    std::vector<double> cum((size_t)N);
    double run = 0.0;
    for (int p = 0; p < N; ++p) {
        run += rho[order[(size_t)p]];
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

// out: con_out_doubles(nc, np, G) doubles
inline void con_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const int32_t* cols, int nc, const double* probs, int np, int G, double scale,
                       double* out)
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
    const int status = mce_mar::mar_status(badw, badcol, W, rows, &column);
    con_pack_head(status, column, W, A2, rows, G, np, nc, out);
    const int P = con_npairs(nc), N = G * G;
    const int64_t total = con_out_doubles(nc, np, G) - kConHead;
    double* col = out + kConHead;
    for (int64_t k = 0; k < total; ++k) col[k] = nan;
    for (int t = 0; t < nc; ++t) col[kConCol * nc + t] = (double)cols[t];
    if (status != mce_mar::kMarOk) return;
    double* pair = col + (int64_t)kConPerCol * nc;
    double* per_p = pair + (int64_t)kConPerPair * P;
    double* dens = per_p + (int64_t)kConPerP * np * P;
    std::vector<double> h((size_t)nc), c((size_t)nc), lo((size_t)nc), step((size_t)nc);
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
        cs[(size_t)t] = con_params(W, A2, V / W, mn, mx, scale, G, &sd, &h[(size_t)t], &c[(size_t)t], &lo[(size_t)t], &step[(size_t)t]);
        col[kConColStatus * nc + t] = (double)cs[(size_t)t];
        if (cs[(size_t)t] != kConOk) continue;
        col[kConMean * nc + t] = m;
        col[kConVar * nc + t] = V / W;
        col[kConSd * nc + t] = sd;
        col[kConH * nc + t] = h[(size_t)t];
        col[kConC * nc + t] = c[(size_t)t];
        col[kConLo * nc + t] = lo[(size_t)t];
        col[kConStep * nc + t] = step[(size_t)t];
    }
    std::vector<double> ex(used.size() * (size_t)G), ey(used.size() * (size_t)G), dec((size_t)(kConPerP * (np > 0 ? np : 1)));
    for (int s = 0; s < nc; ++s) {
        // a_r * E_s[r][kx], once per x axis
        if (cs[(size_t)s] == kConOk)
            for (size_t q = 0; q < used.size(); ++q)
                for (int k = 0; k < G; ++k)
                    ex[q * G + k] = con_weighted(w[used[q]], con_value(c[(size_t)s], mce_mar::mar_grid_point(lo[(size_t)s], step[(size_t)s], k), x[used[q] * ld + cols[s]]));
        for (int t = s + 1; t < nc; ++t) {
            const int p = con_pair_index(s, t, nc);
            const bool ok = cs[(size_t)s] == kConOk && cs[(size_t)t] == kConOk;
            pair[kConPairStatus * P + p] = ok ? (double)kConOk : (double)kConColBad;
            if (!ok) {
                for (int q = 0; q < np; ++q) per_p[(q * kConPerP + kConCells) * P + p] = -1.0;
                continue;
            }
            for (size_t q = 0; q < used.size(); ++q)
                for (int k = 0; k < G; ++k)
                    ey[q * G + k] = con_value(c[(size_t)t], mce_mar::mar_grid_point(lo[(size_t)t], step[(size_t)t], k), x[used[q] * ld + cols[t]]);
            double* rho = dens + (int64_t)p * N;
            const double norm = con_norm(W, h[(size_t)s], h[(size_t)t]);
            for (int kx = 0; kx < G; ++kx)
                for (int ky = 0; ky < G; ++ky) {
                    double acc = 0.0;
                    for (size_t q = 0; q < used.size(); ++q) acc = con_add(acc, ex[q * G + kx], ey[q * G + ky]);
                    rho[kx * G + ky] = acc / norm;
                }
            double mode[3];
            con_decide(rho, G, lo[(size_t)s], step[(size_t)s], lo[(size_t)t], step[(size_t)t], probs, np, mode, dec.data());
            pair[kConModeX * P + p] = mode[0];
            pair[kConModeY * P + p] = mode[1];
            pair[kConModeDensity * P + p] = mode[2];
            for (int q = 0; q < np; ++q)
                for (int z = 0; z < kConPerP; ++z) per_p[(q * kConPerP + z) * P + p] = dec[(size_t)(q * kConPerP + z)];
        }
    }
}

}  // namespace mce_con
#endif
