// jack_groups.hpp -- the bookkeeping of the delete-a-group jackknife for chains that stay on the device (docs/design/jackknife_resident.md):
// the group of every row, and the leave-one-group-out row counts, weight sums and likelihood moments.  Shared by the host check
// (tests/native/jack_groups_check.cpp, plain C++17 under g++) and the device kernels (jack_group_kernels.hpp, __host__ __device__ under
// hipcc), after the pattern of jack.hpp and like_moments.hpp.  mcevidence_amd/jackknife.py (group_ids) and information.py
// (leave_one_out) restate the two halves in NumPy.
//
// GROUP OF A ROW.  Row i of a system is the gathered position i; r = rows[i] under an explicit row list, else i, is its index in the
// burned, concatenated, thinned sample of N rows.
//   by = kJgBlocks   g = r G / N in 64-bit integers (jack.hpp: jack_block_group)
//   by = kJgChains   s = src[r] (the kept row's number in the burned, concatenated numbering), or r when nothing was thinned; g = the
//                    last part whose first row part_first[p] is at or below s (chain_farm.hpp: last_at_or_below; an empty part shares
//                    its first row with the next one and is never the answer).  G is the number of parts.
// An r outside [0, N) gives kJgNoGroup = -1, which every consumer refuses.
//
// LEAVE-ONE-GROUP-OUT BLOCK.  Slot 0 deletes nothing (b = -1), slot 1 + b deletes group b; a slot is taken over the rows with g != b:
//   nrows   every such row (zero-weight rows count: the jackknife's S_b)
//   SumW    sum a over them
//   W, c, v, A2, rows used, status      like_moments.hpp's rule on that set, when an fs column is given: its row test (a == 0 is
//           skipped and its f never read into a sum), its statuses 0 / 3 / 5, NaN values where the status is not 0, and v in a second
//           pass centred on the slot's OWN computed c.  Without an fs column: NaN values and status kJgNoMoments.
// Every leave-out sum is a sum of the deleted set's own terms: additions only, never total - group, so the bound of
// docs/design/information.md holds for every slot at its own n.
// Here:
//   * jg_group              the group of a row;
//   * jg_in_slot            does a row of group g count in slot b's set?
//   * jg_pack               the result block of a slot;
//   * jg_groups_serial, jg_leave_out_serial     the serial drivers: the whole rule on one CPU thread.
#pragma once

#include <stdint.h>

#include "chain_farm.hpp"
#include "jack.hpp"
#include "like_moments.hpp"

#ifndef MCE_JACK_LEAVE_OUT
#define MCE_JACK_LEAVE_OUT 8
#endif

namespace mce_jg {

enum : int { kJgBlocks = 0, kJgChains = 1 };
enum : int { kJgNoGroup = -1 };
enum : int { kJgNoMoments = -1 };         // the status of a slot of a system without an fs column
enum : int { kJgNrows = 0, kJgSumW, kJgW, kJgC, kJgV, kJgA2, kJgUsed, kJgStatus, kJgOut };
static_assert(kJgOut == MCE_JACK_LEAVE_OUT, "the result block of include/mcevidence_hip.h");

// rows, src: NULL or arrays (src has N entries); part_first[nparts]: the parts' first rows in the burned, concatenated numbering
MCE_HD inline int32_t jg_group(int64_t i, const int64_t* rows, const int64_t* src, const int64_t* part_first, int64_t nparts, int64_t N, int64_t G,
                               int by)
{
    const int64_t r = rows ? rows[i] : i;
    if (r < 0 || r >= N) return kJgNoGroup;
    if (by == kJgBlocks) return (int32_t)mce_jack::jack_block_group(r, G, N);
    const int64_t s = src ? src[r] : r;
    if (s < part_first[0]) return kJgNoGroup;
    return (int32_t)mce_farm::last_at_or_below(part_first, nparts, s);
}

// b = -1: nothing is deleted
MCE_HD inline bool jg_in_slot(int g, int b) { return g != b; }

MCE_HD inline void jg_pack(bool moments, double nrows, double sumw, int status, double W, double c, double v, double A2, double used, double* out)
{
    const double nan = __builtin_nan("");
    double m[mce_mom::kMomOut];
    mce_mom::mom_pack(status, W, c, v, A2, used, m);
    out[kJgNrows] = nrows;
    out[kJgSumW] = sumw;
    out[kJgW] = moments ? m[mce_mom::kMomW] : nan;
    out[kJgC] = moments ? m[mce_mom::kMomC] : nan;
    out[kJgV] = moments ? m[mce_mom::kMomV] : nan;
    out[kJgA2] = moments ? m[mce_mom::kMomA2] : nan;
    out[kJgUsed] = moments ? used : nan;
    out[kJgStatus] = moments ? (double)status : (double)kJgNoMoments;
}

// ---- the serial drivers (host): rows in order ------------------------------------------------------------------------------------
inline void jg_groups_serial(const int64_t* rows, const int64_t* src, const int64_t* part_first, int64_t nparts, int64_t n, int64_t N, int64_t G, int by,
                             int32_t* out)
{
    for (int64_t i = 0; i < n; ++i) out[i] = jg_group(i, rows, src, part_first, nparts, N, G, by);
}

// out[(G + 1) * kJgOut]; fs may be NULL.  Returns false (and leaves out untouched) where a group id lies outside [0, G).
inline bool jg_leave_out_serial(const double* w, const double* fs, const int32_t* g, int64_t n, int G, double* out)
{
    for (int64_t i = 0; i < n; ++i)
        if (g[i] < 0 || g[i] >= G) return false;
    for (int b = -1; b < G; ++b) {
        double nrows = 0.0, W = 0.0, S = 0.0, A2 = 0.0, used = 0.0;
        bool bad = false;
        for (int64_t i = 0; i < n; ++i) {
            if (!jg_in_slot(g[i], b)) continue;
            nrows += 1.0;
            const double a = w[i];
            if (!mce_mom::mom_used(a)) continue;
            W += a;
            A2 += a * a;
            used += 1.0;
            if (fs) {
                const double f = fs[i];
                bad = bad || mce_mom::mom_row_bad(a, f);
                S += a * f;
            }
        }
        const int status = mce_mom::mom_status(bad, W);
        const double c = S / W;
        double V = 0.0;
        if (fs && status == mce_mom::kMomOk)
            for (int64_t i = 0; i < n; ++i)
                if (jg_in_slot(g[i], b) && mce_mom::mom_used(w[i])) V += mce_mom::mom_term(w[i], fs[i], c);
        jg_pack(fs != nullptr, nrows, W, status, W, c, V / W, A2, used, out + (int64_t)(b + 1) * kJgOut);
    }
    return true;
}

}  // namespace mce_jg
