// eig_jacobi.hpp -- the symmetric eigen-solvers of the evidence feed and the rules they share, after the pattern of
// chain_prep.hpp / chain_farm.hpp: plain C++17 under g++ (tests/native/eig_jacobi_check.cpp), __host__ __device__ under hipcc
// (eig_kernels.hpp).
//
//   * jacobi_eig            the host solver of the feed (cyclic order, one core), as it always was;
//   * slots / pair_of       the pair schedule of the batched solver: a round-robin tournament over m = d + (d & 1) slots,
//                           m - 1 steps per sweep, m / 2 disjoint pairs per step; a pair with the padding slot is a bye;
//   * rotation              (c, s) from one (a_pp, a_qq, a_pq) with jacobi_eig's formulas and its per-element stopping rule;
//   * rank_of / sign_of     the canonical form: eigenvalues descending in the order of a stable sort, each eigenvector's first
//                           largest-magnitude component positive;
//   * status_of             0 ok, 1 not finite, 2 an eigenvalue that is not > 0 (with its index);
//   * tournament_eig        the serial driver: the device's schedule and phases on one CPU thread.
// The disjoint rotations of one step commute exactly, so a step computes all its angles from the matrix as it stands at the
// start of the step and then applies A <- A J, A <- J^T A and V <- V J for all of them.
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

#include <algorithm>
#include <cmath>
#include <vector>

namespace mce_eig {

constexpr int kMaxSweeps = 100;          // hard cap of both solvers
constexpr double kSkipRel = 1e-16;       // a rotation is skipped when |a_pq| <= kSkipRel sqrt(|a_pp a_qq|)

enum : int { kStatusOk = 0, kStatusNotFinite = 1, kStatusNotPositive = 2 };
// what a solve reports per system (int32 each): the status, the index of the offending eigenvalue (status 2; else 0), the
// sweeps it ran and the rotations it applied
enum : int { kStatCode = 0, kStatIndex = 1, kStatSweeps = 2, kStatRotations = 3, kStatInts = 4 };

// cyclic Jacobi eigen-solver for a symmetric d x d matrix (row-major A, destroyed); eigenvalues in
// lam[d], eigenvectors in the COLUMNS of V (row-major [d][d]).  d <= 1024.  Per-element stopping rule
// (Demmel & Veselic 1992): a rotation is skipped when |a_pq| <= 1e-16 sqrt(a_pp a_qq), and the solver stops
// after a sweep without one.  Every eigenvalue then carries a RELATIVE error of about eps * cond(Cn), Cn the
// correlation matrix diag(A)^-1/2 A diag(A)^-1/2 -- the accuracy A's own rounding allows -- however graded A is.
// (A rule relative to the whole diagonal, off(A) <= 1e-32 |diag A|^2, stops while the smallest eigenvalues of a
// graded covariance are still wrong by 2e-9 relative, and by up to 9e-4 on few rows: tests/test_gpu_feeders.py.)
inline void jacobi_eig(std::vector<double>& A, int d, std::vector<double>& lam, std::vector<double>& V)
{
    V.assign((size_t)d * d, 0.0);
    for (int i = 0; i < d; ++i) V[(size_t)i * d + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < d - 1; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = A[(size_t)p * d + q];
                if (std::fabs(apq) <= 1e-16 * std::sqrt(std::fabs(A[(size_t)p * d + p] * A[(size_t)q * d + q]))) continue;
                rotated = true;
                const double app = A[(size_t)p * d + p], aqq = A[(size_t)q * d + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < d; ++k) {          // A <- A J   (columns p, q)
                    const double akp = A[(size_t)k * d + p], akq = A[(size_t)k * d + q];
                    A[(size_t)k * d + p] = c * akp - s * akq;
                    A[(size_t)k * d + q] = s * akp + c * akq;
                }
                for (int k = 0; k < d; ++k) {          // A <- J^T A (rows p, q)
                    const double apk = A[(size_t)p * d + k], aqk = A[(size_t)q * d + k];
                    A[(size_t)p * d + k] = c * apk - s * aqk;
                    A[(size_t)q * d + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < d; ++k) {          // V <- V J
                    const double vkp = V[(size_t)k * d + p], vkq = V[(size_t)k * d + q];
                    V[(size_t)k * d + p] = c * vkp - s * vkq;
                    V[(size_t)k * d + q] = s * vkp + c * vkq;
                }
            }
        if (!rotated) break;
    }
    // canonical form: eigenvalues descending, each eigenvector's largest component positive.  Two
    // sets whitened with their OWN systems (covtype 'single' cross evidence) are then rotated
    // consistently whenever their covariances are close, whatever the sweep order did.
    std::vector<int> order(d);
    for (int i = 0; i < d; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * d + a] > A[(size_t)b * d + b]; });
    lam.resize(d);
    std::vector<double> Vs((size_t)d * d);
    for (int c = 0; c < d; ++c) {
        const int src = order[c];
        lam[c] = A[(size_t)src * d + src];
        int big = 0;
        for (int k = 1; k < d; ++k)
            if (std::fabs(V[(size_t)k * d + src]) > std::fabs(V[(size_t)big * d + src])) big = k;
        const double sgn = V[(size_t)big * d + src] < 0.0 ? -1.0 : 1.0;
        for (int k = 0; k < d; ++k) Vs[(size_t)k * d + c] = sgn * V[(size_t)k * d + src];
    }
    V.swap(Vs);
}

// ---- the pair schedule ------------------------------------------------------------------------------------------------------
MCE_HD inline int slots(int d) { return d + (d & 1); }
MCE_HD inline int steps_per_sweep(int d) { return slots(d) - 1; }
MCE_HD inline int pairs_per_step(int d) { return slots(d) / 2; }
// pair k of step `step` (circle method: slot m - 1 stays, the others turn): p < q; q >= d is a bye (d odd: the padding slot)
MCE_HD inline void pair_of(int d, int step, int k, int& p, int& q)
{
    const int m = slots(d), r = m - 1;
    int a, b;
    if (k == 0) {
        a = m - 1;
        b = step;
    } else {
        a = step + k;
        if (a >= r) a -= r;
        b = step - k;
        if (b < 0) b += r;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// ---- the rotation -----------------------------------------------------------------------------------------------------------
MCE_HD inline bool is_finite(double x) { return x - x == 0.0; }
// false: skip (the per-element stopping rule); true: J = [c s; -s c] annihilates a_pq
MCE_HD inline bool rotation(double app, double aqq, double apq, double& c, double& s)
{
    if (fabs(apq) <= kSkipRel * sqrt(fabs(app * aqq))) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    c = 1.0 / sqrt(t * t + 1.0);
    s = t * c;
    return true;
}
MCE_HD inline void rotate(double c, double s, double& xp, double& xq)
{
    const double a = xp, b = xq;
    xp = c * a - s * b;
    xq = s * a + c * b;
}

// ---- the canonical form -----------------------------------------------------------------------------------------------------
// position of eigenvalue i in descending order, ties in index order (what std::stable_sort gives): rank by counting
MCE_HD inline int rank_of(const double* lam, int d, int i)
{
    int r = 0;
    const double x = lam[i];
    for (int j = 0; j < d; ++j) r += (lam[j] > x || (lam[j] == x && j < i)) ? 1 : 0;
    return r;
}
// sign that makes the first largest-magnitude component of column `col` of V (row-major, leading dimension ld) positive
MCE_HD inline double sign_of(const double* V, int d, int ld, int col)
{
    int big = 0;
    for (int k = 1; k < d; ++k)
        if (fabs(V[(size_t)k * ld + col]) > fabs(V[(size_t)big * ld + col])) big = k;
    return V[(size_t)big * ld + col] < 0.0 ? -1.0 : 1.0;
}

// ---- the status rule --------------------------------------------------------------------------------------------------------
// of the SORTED eigenvalues: the first that is not finite gives 1, the first that is not > 0 gives 2 and its index
MCE_HD inline int status_of(const double* lam_sorted, int d, int& index)
{
    index = 0;
    for (int i = 0; i < d; ++i) {
        if (!is_finite(lam_sorted[i])) return kStatusNotFinite;
        if (!(lam_sorted[i] > 0.0)) {
            index = i;
            return kStatusNotPositive;
        }
    }
    return kStatusOk;
}

// ---- the serial driver ------------------------------------------------------------------------------------------------------
// What eig_kernels.hpp does for one system, on one thread: cov[d*d] (row-major, untouched) -> evec[d*d] (eigenvectors in the
// columns), scale[d] = 1 / sqrt(lam), lam[d] (descending), stat[kStatInts].  A system that is not status 0 still gets finite
// evec (identity) and scale (1); lam then holds what the sweeps left (status 2) or the input's diagonal (status 1).
inline void tournament_eig(const double* cov, int d, double* evec, double* scale, double* lam, int32_t* stat)
{
    std::vector<double> A(cov, cov + (size_t)d * d), V((size_t)d * d, 0.0);
    bool finite = true;
    for (double x : A) finite = finite && is_finite(x);
    int sweeps = 0, rotations = 0, code = kStatusOk, index = 0;
    if (!finite) {
        code = kStatusNotFinite;
        for (int i = 0; i < d; ++i) lam[i] = A[(size_t)i * d + i];
    } else {
        for (int i = 0; i < d; ++i) V[(size_t)i * d + i] = 1.0;
        const int np = pairs_per_step(d);
        std::vector<double> cs(np), sn(np);
        std::vector<int> pp(np), qq(np);
        std::vector<char> on(np);
        for (; sweeps < kMaxSweeps;) {
            bool rotated = false;
            for (int step = 0; step < steps_per_sweep(d); ++step) {
                bool any = false;
                for (int k = 0; k < np; ++k) {                                   // phase 1: the angles, from the matrix as it stands
                    pair_of(d, step, k, pp[k], qq[k]);
                    on[k] = qq[k] < d && rotation(A[(size_t)pp[k] * d + pp[k]], A[(size_t)qq[k] * d + qq[k]], A[(size_t)pp[k] * d + qq[k]], cs[k], sn[k]);
                    any = any || on[k];
                    rotations += on[k] ? 1 : 0;
                }
                if (!any) continue;
                rotated = true;
                for (int k = 0; k < np; ++k)                                     // phase 2: A <- A J
                    if (on[k])
                        for (int r = 0; r < d; ++r) rotate(cs[k], sn[k], A[(size_t)r * d + pp[k]], A[(size_t)r * d + qq[k]]);
                for (int k = 0; k < np; ++k)                                     // phase 3: A <- J^T A
                    if (on[k])
                        for (int r = 0; r < d; ++r) rotate(cs[k], sn[k], A[(size_t)pp[k] * d + r], A[(size_t)qq[k] * d + r]);
                for (int k = 0; k < np; ++k)                                     // phase 4: V <- V J
                    if (on[k])
                        for (int r = 0; r < d; ++r) rotate(cs[k], sn[k], V[(size_t)r * d + pp[k]], V[(size_t)r * d + qq[k]]);
            }
            ++sweeps;
            if (!rotated) break;
        }
        std::vector<double> diag(d), sorted(d);
        std::vector<int> rank(d);
        for (int i = 0; i < d; ++i) diag[i] = A[(size_t)i * d + i];
        for (int i = 0; i < d; ++i) {
            rank[i] = rank_of(diag.data(), d, i);
            sorted[rank[i]] = diag[i];
        }
        code = status_of(sorted.data(), d, index);
        for (int i = 0; i < d; ++i) lam[i] = sorted[i];
        if (code == kStatusOk)
            for (int i = 0; i < d; ++i) {
                const double sgn = sign_of(V.data(), d, d, i);
                for (int k = 0; k < d; ++k) evec[(size_t)k * d + rank[i]] = sgn * V[(size_t)k * d + i];
                scale[rank[i]] = 1.0 / std::sqrt(diag[i]);
            }
    }
    if (code != kStatusOk)
        for (int i = 0; i < d; ++i) {
            for (int k = 0; k < d; ++k) evec[(size_t)k * d + i] = k == i ? 1.0 : 0.0;
            scale[i] = 1.0;
        }
    stat[kStatCode] = code;
    stat[kStatIndex] = index;
    stat[kStatSweeps] = sweeps;
    stat[kStatRotations] = rotations;
}

}  // namespace mce_eig
