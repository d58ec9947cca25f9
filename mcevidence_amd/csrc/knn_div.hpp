// knn_div.hpp -- the k-NN relative entropy D_KL(P || Q) of two weighted samples and its delete-a-group jackknife from ONE pair of
// neighbour searches (docs/design/knn_divergence.md), shared by the host check (tests/native/div_check.cpp, plain C++17 under g++) and
// the device kernels (knn_div_kernels.hpp, __host__ __device__ under hipcc), after the pattern of jack.hpp, whose list walk it reuses.
// mcevidence_amd/divergence.py (measure) restates it in NumPy.
//
// P = (xp[nP][d], a[nP]) and Q = (xq[nQ][d], b[nQ]) are whitened with P's system (div_whiten_coord).  Every P row i has two ascending
// lists of L entries (distance, row): the AUTO list (its neighbours among the other P rows; the own row, where the list holds it, is
// skipped) and the CROSS list (its neighbours in Q).  With b the deleted group (b = -1: none), a row i with gP[i] != b and a rank
// k = 1 .. K, both lists walked with entries of group b skipped (jack_entry_group / jack_keep / jack_next):
//   rho, MA = the distance of the k-th kept auto entry and the sum of the weights a of the first k kept auto entries, in list order
//   nu,  MB = the same of the cross list with the weights b
//   WP_b    = W_P - (the weight of P's group b),  WP_{-1} = W_P
//   s       = d (log nu - log rho) + log MA - log MB - log(WP_b - a_i)
//   N[b][k] = sum a_i s     over the rows that enter with rho > 0 and nu > 0
//   X[b][k] = sum a_i       over the rows that enter with rho == 0 or nu == 0 (coincident rows: they enter X and not N)
//   D[b][k] = N[b][k] / (WP_b - X[b][k]) + log WQ_b
// A row is SHORT (jack.hpp's definition, applied to either list) when skipping some group other than its own, or none, leaves fewer
// than K entries in the auto list or in the cross list: it enters no sum and is handed back for longer lists.  G = 0: no groups, the
// full slot alone.
// Here:
//   * div_whiten_coord        coordinate k of z = Linv (x - m), the products added in column order
//   * div_entry_group         the group an entry counts under (group 0 where there are no groups)
//   * div_is_short            the short test over both lists
//   * div_s, div_coincident   the term of a rank, and whether the rank is a coincident one
//   * div_value               D from N, X and the two masses
//   * div_masses              W and the group weights of a sample, added in row order
//   * div_serial              the serial driver: all sums and the short rows on one CPU thread
#pragma once

#include "jack.hpp"

namespace mce_div {

using mce_jack::JackCursor;
using mce_jack::jack_entry_group;
using mce_jack::jack_keep;
using mce_jack::jack_next;
using mce_jack::jack_runs_out;
using mce_jack::kJackSkip;

constexpr int kDivMaxK = 16;             // == MCE_DIV_MAX_K: ranks of the sums
constexpr int kDivMaxDim = 64;           // == MCE_DIV_MAX_DIM: columns (the Cholesky factor travels with the call)
constexpr int kDivMaxList = 1024;        // the longest list (== MCE_GENERIC_MAX_K)
constexpr int kDivReport = 4;            // == MCE_DIV_REPORT: sum of w, weights that are not > 0 or not finite, lowest non-finite column, rows

#define MCE_DIV_NO_CONTRACT _Pragma("clang fp contract(off)")

// coordinate k of a whitened row: y_j = x_j - mean_j, the products added in column order (no fused multiply-add: NumPy has none)
MCE_HD inline double div_whiten_coord(const double* lrow, const double* x, const double* mean, int k)
{
#if defined(__clang__)
    MCE_DIV_NO_CONTRACT
#endif
    double acc = 0.0;
    for (int j = 0; j <= k; ++j) {
        const double y = x[j] - mean[j];
        const double p = lrow[j] * y;
        acc = acc + p;
    }
    return acc;
}

MCE_HD inline bool div_finite(double v) { return v - v == 0.0; }
MCE_HD inline bool div_bad_weight(double w) { return !(w > 0.0) || !div_finite(w); }

// gr NULL (G = 0): every entry that exists counts under group 0
MCE_HD inline int div_entry_group(int64_t idx, int64_t nr, const int32_t* gr, int64_t self)
{
    if (gr) return jack_entry_group(idx, nr, gr, self);
    return (idx < 0 || idx >= nr || idx == self) ? kJackSkip : 0;
}

template <class GroupA, class GroupB>
MCE_HD inline bool div_is_short(GroupA group_a, GroupB group_b, int L, int own, int G, int K)
{
    if (jack_runs_out(group_a, L, -1, K) || jack_runs_out(group_b, L, -1, K)) return true;
    for (int b = 0; b < G; ++b)
        if (b != own && (jack_runs_out(group_a, L, b, K) || jack_runs_out(group_b, L, b, K))) return true;
    return false;
}

// log rho / log nu of a coincident rank is log 0
MCE_HD inline bool div_coincident(double lrho, double lnu) { return lrho == -INFINITY || lnu == -INFINITY; }

// lw = log(WP_b - a_i)
MCE_HD inline double div_s(int d, double lnu, double lrho, double MA, double MB, double lw)
{
#if defined(__clang__)
    MCE_DIV_NO_CONTRACT
#endif
    const double t = (double)d * (lnu - lrho);
    return t + log(MA) - log(MB) - lw;
}

MCE_HD inline double div_value(double N, double X, double WPb, double WQb) { return N / (WPb - X) + log(WQb); }

#if !defined(__HIP_DEVICE_COMPILE__)
// out[0] = the sum of a, out[1 + g] = the sum of a over the rows of group g, both in row order
inline void div_masses(const double* a, const int32_t* g, int64_t n, int G, double* out)
{
    for (int s = 0; s <= G; ++s) out[s] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        out[0] += a[i];
        if (G > 0) out[1 + g[i]] += a[i];
    }
}

// The serial driver.  distP / idxP, distQ / idxQ: [nq][L]; qid: the rows' own P rows (NULL: row q is P row q), skipped in the auto list
// and reported in short_rows; gq / aq: [nq]; grP / aP: [nP]; grQ / bQ: [nQ] (the groups NULL where G = 0).  sums: [(G + 1)][K][2],
// slot 0 the full sample, slot 1 + b group b, N then X; short_rows: [nq], ascending.  Returns the number of short rows.
inline int64_t div_serial(const double* distP, const int64_t* idxP, const double* distQ, const int64_t* idxQ, int64_t nq, int L, const int64_t* qid,
                          const int32_t* gq, const int32_t* grP, int64_t nP, const int32_t* grQ, int64_t nQ, int G, int K, int d, const double* aq,
                          const double* aP, const double* bQ, double* sums, int64_t* short_rows)
{
    double wp[mce_jack::kJackMaxGroups + 1];
    div_masses(aP, grP, nP, G, wp);
    for (int i = 0; i < (G + 1) * K * 2; ++i) sums[i] = 0.0;
    int64_t nshort = 0;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t self = qid ? qid[q] : q;
        const int64_t *ia = idxP + q * (int64_t)L, *ib = idxQ + q * (int64_t)L;
        const double *da = distP + q * (int64_t)L, *db = distQ + q * (int64_t)L;
        const int own = G > 0 ? gq[q] : -2;          // (no groups: no slot is the row's own)
        auto group_a = [&](int j) { return div_entry_group(ia[j], nP, G > 0 ? grP : nullptr, self); };
        auto group_b = [&](int j) { return div_entry_group(ib[j], nQ, G > 0 ? grQ : nullptr, -1); };
        if (div_is_short(group_a, group_b, L, own, G, K)) {
            short_rows[nshort++] = self;
            continue;
        }
        for (int b = -1; b < G; ++b) {
            if (b == own) continue;
            const double lw = log((b < 0 ? wp[0] : wp[0] - wp[1 + b]) - aq[q]);
            double* out = sums + (int64_t)(b + 1) * K * 2;
            JackCursor ca, cb;
            double MA = 0.0, MB = 0.0;
            for (int k = 0; k < K; ++k) {
                const int ja = jack_next(group_a, L, b, ca), jb = jack_next(group_b, L, b, cb);
                MA += aP[ia[ja]];
                MB += bQ[ib[jb]];
                const double lrho = log(da[ja]), lnu = log(db[jb]);
                if (div_coincident(lrho, lnu)) out[2 * k + 1] += aq[q];
                else out[2 * k] += aq[q] * div_s(d, lnu, lrho, MA, MB, lw);
            }
        }
    }
    return nshort;
}
#endif

}  // namespace mce_div
