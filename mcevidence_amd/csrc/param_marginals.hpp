// param_marginals.hpp -- the 1-D marginal posterior densities behind marginals= (a Gaussian kernel density estimate of every parameter
// column on a regular grid, its mode and its highest-posterior-density regions), shared by the host check
// (tests/native/param_marginals_check.cpp, plain C++17 under g++) and the device kernels (param_marginals_kernels.hpp,
// __host__ __device__ under hipcc), after the pattern of param_summary.hpp.  docs/design/marginals.md states the rule;
// mcevidence_amd/marginals.py (measure) restates it in NumPy.
//
// A SYSTEM is one (x, ld, n, d, w): a_i = w[i], x_ij = x[i * ld + j] for j < d (raw, unwhitened) of the s1 partition the estimator
// sums over.  A row with a_i == 0 is skipped entirely.  All in fp64, G grid points, a bandwidth scale s:
//   1  W, A2, m_j, v_j (a second pass about the computed m_j), min_j, max_j as param_summary.hpp forms them;  ess = W * W / A2,
//      sd_j = sqrt(v_j)
//   2  h_j = (s * sd_j) * pow(4 / (3 * ess), 0.2),   c_j = 1 / ((2 * h_j) * h_j)
//   3  lo_j = min_j - 3 * h_j,  hi_j = max_j + 3 * h_j,  step_j = (hi_j - lo_j) / (G - 1),  g_k = lo_j + k * step_j (a product and a
//      sum, two roundings: never one fused operation)
//   4  S_jk = sum over used i of a_i K(c_j (g_k - x_ij)^2),  K(arg) = arg >= 746 ? +0.0 : exp(-arg)  (kde_shift.hpp's
//      kde_kernel_arg_value),   rho_jk = S_jk / ((W * h_j) * sqrt(2 pi))
//   5  mode: the grid point with the largest rho, the lowest k among equals
//   6  for a probability p: the G points ordered by rho descending, then k ascending; rho accumulated SERIALLY in that order, Z the
//      final running sum; selected = the positions up to and including the first whose running sum is >= p * Z (none: all);
//      lower / upper = the smallest / largest selected g, pieces = the maximal runs of consecutive selected k, edge = 1 where k = 0 or
//      k = G - 1 is selected
// The densities are DEFINED at the reported h, c, lo and step.  status of a system: param_summary.hpp's 3 and 5 in its precedence,
// then 6: fewer than 2 used rows; with a status other than 0 every value is NaN.  col_status of a column: 7 where sd_j is 0 or h_j, c_j
// or step_j is not finite and > 0; such a column is NaN, its pieces -1, and the other columns do not notice.
// Here:
//   * mar_grid_ok, mar_nparts, mar_part_tile                     the grids the rule takes; how the device cuts a system's rows: by n alone;
//   * mar_params                                                 steps 2 and 3 and the column's status;
//   * mar_grid_point, mar_arg, mar_add, mar_norm                 the pieces of steps 3 and 4 as every route rounds them;
//   * mar_before                                                 the order of step 6;
//   * mar_status, the result block's layout (kMar.., mar_out_doubles);
//   * mar_decide                                                 steps 5 and 6 on a density array: serial, so bit-reproducible;
//   * mar_serial                                                 the serial driver: the whole rule on one CPU thread
//     (both forward to the one text of param_marginals_bounds.hpp, which serves the rule with bounds too).
#pragma once

#include <stdint.h>

#include <cmath>

#include "kde_shift.hpp"
#include "param_summary.hpp"
#include "seg_tiles.hpp"

#ifndef MCE_MARGINALS_HEAD
#define MCE_MARGINALS_HEAD 8
#endif
#ifndef MCE_MARGINALS_MAX_P
#define MCE_MARGINALS_MAX_P 7
#endif

namespace mce_mar {

enum : int { kMarOk = 0, kMarNotFinite = 3, kMarNoWeight = 5, kMarFewRows = 6, kMarColBad = 7 };
// the head of a result block
enum : int { kMarW = 0, kMarA2, kMarRows, kMarStatus, kMarColumn, kMarGrid, kMarNp, kMarReserved, kMarHead };
static_assert(kMarHead == MCE_MARGINALS_HEAD, "the result block of include/mcevidence_hip.h");
// the per-column rows after the head, d doubles each; then, per probability, kMarPerP rows of d; then density[d][G]
enum : int { kMarMean = 0, kMarVar, kMarSd, kMarH, kMarC, kMarLo, kMarStep, kMarMode, kMarModeDensity, kMarColStatus, kMarPerCol };
enum : int { kMarLower = 0, kMarUpper, kMarPieces, kMarEdge, kMarPerP };
constexpr int kMarMaxDim = mce_sum::kSumMaxDim;
constexpr int kMarMaxP = MCE_MARGINALS_MAX_P;
constexpr int kMarMaxGrid = 1024;
constexpr int kMarMaxParts = 64;                                // parts of a system's rows
constexpr int kMarBlock = 256;                                  // grid points of a workgroup
constexpr double kMarSqrt2Pi = 2.5066282746310002;              // sqrt(2 pi), rounded to nearest

MCE_HD inline bool mar_grid_ok(int G) { return G == 64 || G == 128 || G == 256 || G == 512 || G == 1024; }
MCE_HD inline int64_t mar_out_doubles(int d, int np, int G) { return (int64_t)kMarHead + (int64_t)d * (kMarPerCol + kMarPerP * np + G); }
MCE_HD inline int mar_nblocks(int G) { return (G + kMarBlock - 1) / kMarBlock; }
MCE_HD inline int mar_nparts(int64_t n)
{
    const int64_t t = mce_seg::seg_ntiles(n);
    return t < kMarMaxParts ? (int)t : kMarMaxParts;
}
// the first tile of part p (p = nparts: the end)
MCE_HD inline int64_t mar_part_tile(int64_t n, int p)
{
    const int np = mar_nparts(n);
    return np > 0 ? mce_seg::seg_ntiles(n) * p / np : 0;          // (a system without rows has no part)
}

MCE_HD inline bool mar_pos_finite(double v) { return v > 0.0 && v - v == 0.0; }

// The pieces that carry a product next to a sum are kept from being fused: their roundings are part of the rule.
#if defined(__clang__)
#define MCE_MAR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MCE_MAR_NO_CONTRACT
#endif

// steps 2 and 3 -> the column's status
MCE_HD inline int mar_params(double W, double A2, double v, double mn, double mx, double scale, int G, double* sd, double* h, double* c, double* lo, double* step)
{
    MCE_MAR_NO_CONTRACT
    const double ess = W * W / A2;
    *sd = sqrt(v);
    const double t = 4.0 / (3.0 * ess);
    const double f = pow(t, 0.2);
    const double sc = scale * *sd;
    *h = sc * f;
    const double h2 = 2.0 * *h;
    *c = 1.0 / (h2 * *h);
    const double m3 = 3.0 * *h;
    *lo = mn - m3;
    const double hi = mx + m3;
    const double span = hi - *lo;
    *step = span / (double)(G - 1);
    const bool ok = *sd > 0.0 && mar_pos_finite(*h) && mar_pos_finite(*c) && mar_pos_finite(*step);
    return ok ? kMarOk : kMarColBad;
}

MCE_HD inline double mar_grid_point(double lo, double step, int k)
{
    MCE_MAR_NO_CONTRACT
    const double p = (double)k * step;
    return lo + p;
}
// the argument of one kernel value
MCE_HD inline double mar_arg(double c, double g, double x)
{
    MCE_MAR_NO_CONTRACT
    const double e = g - x;
    const double s = e * e;
    return c * s;
}
// S + a K(arg)
MCE_HD inline double mar_add(double S, double a, double arg)
{
    MCE_MAR_NO_CONTRACT
    const double t = a * mce_kde::kde_kernel_arg_value(arg);
    return S + t;
}
MCE_HD inline double mar_norm(double W, double h)
{
    MCE_MAR_NO_CONTRACT
    const double wh = W * h;
    return wh * kMarSqrt2Pi;
}

// does (rho, k) come before (rho2, k2) in step 6's order?
MCE_HD inline bool mar_before(double rho, int k, double rho2, int k2) { return rho > rho2 || (rho == rho2 && k < k2); }

// the system's status: badw / badcol as param_summary.hpp's sum_status takes them (there is no likelihood here)
MCE_HD inline int mar_status(bool badw, int badcol, double W, double rows, int* column)
{
    const int s = mce_sum::sum_status(badw, false, badcol, W, column);
    if (s != mce_sum::kSumOk) return s;
    return rows < 2.0 ? kMarFewRows : kMarOk;
}

MCE_HD inline void mar_pack_head(int status, int column, double W, double A2, double rows, int G, int np, double* out)
{
    const bool ok = status == kMarOk;
    const double nan = __builtin_nan("");
    out[kMarW] = ok ? W : nan;
    out[kMarA2] = ok ? A2 : nan;
    out[kMarRows] = rows;
    out[kMarStatus] = (double)status;
    out[kMarColumn] = (double)column;
    out[kMarGrid] = (double)G;
    out[kMarNp] = (double)np;
    out[kMarReserved] = 0.0;
}

}  // namespace mce_mar

// ---- the serial drivers (host) --------------------------------------------------------------------------------------------------
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>

namespace mce_mar {

// The drivers are one text for the rule without and with bounds (param_marginals_bounds.hpp, at the end of this file, has them, behind
// the pieces of its rule that they call): mar_decide_ends with the end flags of step 8', mar_serial_bounds with bounds that may be null.
inline void mar_decide_ends(const double* rho, int G, double lo, double step, bool at_lo, bool at_hi, const double* probs, int np, double* mode, double* dec);
inline void mar_serial_bounds(const double* x, int64_t ld, int64_t n, int d, const double* w, const double* bounds, const double* probs, int np, int G, double scale,
                              double* out);

// steps 5 and 6 on the G densities of one column: mode[2] = the mode and its density; dec[p * kMarPerP ..]: lower, upper, pieces, edge
inline void mar_decide(const double* rho, int G, double lo, double step, const double* probs, int np, double* mode, double* dec)
{
    mar_decide_ends(rho, G, lo, step, false, false, probs, np, mode, dec);
}

// out: mar_out_doubles(d, np, G) doubles
inline void mar_serial(const double* x, int64_t ld, int64_t n, int d, const double* w, const double* probs, int np, int G, double scale, double* out)
{
    mar_serial_bounds(x, ld, n, d, w, nullptr, probs, np, G, scale, out);
}

}  // namespace mce_mar
#endif

#include "param_marginals_bounds.hpp"                           // (last: it opens with this file, whichever of the two is named first)
