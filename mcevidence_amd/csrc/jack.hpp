// jack.hpp -- the delete-a-group jackknife of ln E from ONE neighbour search (docs/design/jackknife.md), shared by the host check
// (tests/native/jack_check.cpp, plain C++17 under g++) and the device kernels (jack_kernels.hpp, __host__ __device__ under hipcc),
// after the pattern of chain_corr.hpp / chain_farm.hpp.  mcevidence_amd/jackknife.py (jackknife_host) restates it in NumPy.
//
// Every query row q has an ascending neighbour list of L entries (distance, reference row), a weight w, a shifted log-likelihood fs
// and a group gq in [0, G); every reference row has a group gr.  With K = kmax - k0 and b the deleted group:
//   dotp_b[k] = sum over q with gq[q] != b of  c_q r_{q,b,k}^D,      c_q r^D = sgn(w_q) exp(lnC_D - ln|w_q| + fs_q + D ln r)
//   r_{q,b,k} = the distance of the (k - k0 + 1)-th entry of q's list once entries of group b -- and the row's own entry, where the
//               list holds it (auto evidence, k0 = 1) -- are skipped.
// A row is SHORT when skipping some group b != its own (or no group at all) leaves fewer than K entries: it enters no sum, neither
// a group's nor the full one, and is handed back for a longer list.
// Here:
//   * jack_block_group       the group of a row under by="blocks";
//   * jack_entry_group       the group an entry counts under: its row's, or kJackSkip for a missing entry and for the own row;
//   * jack_keep, jack_next   the list walk: skip group b, skip self, report that the list ran out;
//   * jack_term              the term of an entry, the expression of dotp_partial_kernel;
//   * jack_sigma, jack_bias_corrected     the two formulas over the G leave-one-group-out values;
//   * jack_serial            the serial driver: all sums and the short rows on one CPU thread.
#pragma once

#include <math.h>
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

namespace mce_jack {

constexpr int kJackMaxGroups = 64;      // == MCE_JACK_MAX_GROUPS
constexpr int kJackMaxK = 32;           // == MCE_MAX_K: columns of the sums
constexpr int kJackSkip = 255;          // the "group" of an entry that is never kept

// by="blocks": G contiguous stretches of the N rows of the burned / thinned sample
MCE_HD inline int jack_block_group(int64_t row, int64_t G, int64_t N) { return (int)(row * G / N); }

// idx: the entry's reference row (negative: the list ended); self: the query's own reference row, or -1 where it has none
MCE_HD inline int jack_entry_group(int64_t idx, int64_t nr, const int32_t* gr, int64_t self)
{
    if (idx < 0 || idx >= nr || idx == self) return kJackSkip;
    return (int)gr[idx];
}

MCE_HD inline bool jack_keep(int g, int b) { return g != kJackSkip && g != b; }

struct JackCursor {
    int j = 0;          // next entry to look at
    int kept = 0;       // entries kept so far
};

// the next kept entry of a list whose entry j counts under group group_at(j), with group b deleted (b = -1: none): its position, or
// -1 when the list ran out
template <class GroupAt>
MCE_HD inline int jack_next(GroupAt group_at, int L, int b, JackCursor& c)
{
    while (c.j < L) {
        const int at = c.j++;
        if (jack_keep(group_at(at), b)) {
            ++c.kept;
            return at;
        }
    }
    return -1;
}

// does deleting group b leave fewer than K entries?
template <class GroupAt>
MCE_HD inline bool jack_runs_out(GroupAt group_at, int L, int b, int K)
{
    JackCursor c;
    while (c.kept < K)
        if (jack_next(group_at, L, b, c) < 0) return true;
    return false;
}

template <class GroupAt>
MCE_HD inline bool jack_is_short(GroupAt group_at, int L, int own, int G, int K)
{
    if (jack_runs_out(group_at, L, -1, K)) return true;
    for (int b = 0; b < G; ++b)
        if (b != own && jack_runs_out(group_at, L, b, K)) return true;
    return false;
}

// base = lnC_D - ln|w| + fs, sgn = the sign of w: exactly what dotp_partial_kernel forms
MCE_HD inline double jack_base(double lnc, double w, double fs) { return lnc - log(fabs(w)) + fs; }
MCE_HD inline double jack_term(double sgn, double base, int D, double r) { return sgn * exp(base + (double)D * log(r)); }

// sigma = sqrt((G - 1) / G sum_b (v_b - mean)^2) over the G leave-one-group-out values
MCE_HD inline double jack_mean(const double* v, int G)
{
    double s = 0.0;
    for (int b = 0; b < G; ++b) s += v[b];
    return s / (double)G;
}

MCE_HD inline double jack_sigma(const double* v, int G)
{
    const double m = jack_mean(v, G);
    double s = 0.0;
    for (int b = 0; b < G; ++b) s += (v[b] - m) * (v[b] - m);
    return sqrt((double)(G - 1) / (double)G * s);
}

// G v_full - (G - 1) mean_b v_b
MCE_HD inline double jack_bias_corrected(const double* v, int G, double v_full) { return (double)G * v_full - (double)(G - 1) * jack_mean(v, G); }

#if !defined(__HIP_DEVICE_COMPILE__)
inline double jack_ln_unit_ball(int d) { return 0.5 * d * log(M_PI) - lgamma(1.0 + 0.5 * d); }

// The serial driver.  dist / idx: [nq][L]; qid: the rows' own reference rows (NULL: row q is reference row q), used for the self
// entry when k0 == 1 and reported in short_rows; gq / w / fs: [nq]; gr: [nr].  dotp_groups: [G][kmax], dotp_full: [kmax] (entries
// below k0 are 0); short_rows: [nq], ascending.  Returns the number of short rows.
inline int64_t jack_serial(const double* dist, const int64_t* idx, int64_t nq, int L, const int64_t* qid, const int32_t* gq, const int32_t* gr,
                           int64_t nr, int G, int k0, int kmax, int D, const double* w, const double* fs, double* dotp_groups, double* dotp_full,
                           int64_t* short_rows)
{
    const int K = kmax - k0;
    const double lnc = jack_ln_unit_ball(D);
    for (int i = 0; i < G * kmax; ++i) dotp_groups[i] = 0.0;
    for (int k = 0; k < kmax; ++k) dotp_full[k] = 0.0;
    int64_t nshort = 0;
    for (int64_t q = 0; q < nq; ++q) {
        const int64_t row = qid ? qid[q] : q;
        const int64_t self = k0 == 1 ? row : -1;
        const int64_t* li = idx + q * (int64_t)L;
        const double* ld = dist + q * (int64_t)L;
        auto group_at = [&](int j) { return jack_entry_group(li[j], nr, gr, self); };
        if (jack_is_short(group_at, L, gq[q], G, K)) {
            short_rows[nshort++] = row;
            continue;
        }
        const double base = jack_base(lnc, w[q], fs[q]), sgn = w[q] < 0.0 ? -1.0 : 1.0;
        for (int b = -1; b < G; ++b) {
            if (b == gq[q]) continue;
            double* out = b < 0 ? dotp_full : dotp_groups + (int64_t)b * kmax;
            JackCursor c;
            for (int k = k0; k < kmax; ++k) out[k] += jack_term(sgn, base, D, ld[jack_next(group_at, L, b, c)]);
        }
    }
    return nshort;
}
#endif

}  // namespace mce_jack
