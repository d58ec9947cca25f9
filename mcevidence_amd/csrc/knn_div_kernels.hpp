// knn_div_kernels.hpp -- the k-NN relative entropy's sums on the device (rule: knn_div.hpp; docs/design/knn_divergence.md).  fp64
// throughout, plain vector stores, no floating-point atomics, 64-bit row indices: every sum is a block_sum over 256 rows followed by a
// fixed-order pass over the blocks (jack_final_kernel), so the order of every addition is fixed by the sizes alone.
//
//   div_whiten_kernel          one lane per row: z = Linv (x - m) in the rule's order (the factor and the mean in LDS), packed [n][d];
//                              per block the sum of w, the count of weights that are not > 0 or not finite, the lowest column with a
//                              value that is not finite
//   div_report_kernel          one workgroup folds the blocks' three numbers in block order
//   div_mass_kernel            per block and slot the weight of P: slot 0 every row, slot 1 + b the rows of group b
//   div_terms_kernel<RL>       one lane per query, 256 queries per workgroup.  RL = 16 or 32 (L <= RL): both lists -- the logarithms of
//                              the distances, the gathered weights and the group bytes, four to a word -- are loaded once and stay in
//                              registers; the loops over the deleted group b and the rank k are wave-uniform, and the k-th kept entry of
//                              either list is picked by compare-and-select, as jack_partial_kernel<true> does (no indexed private
//                              array, no scratch).  RL = 0
//                              (the ladder's 128 rung: a handful of rows): both lists are walked from memory in step with jack_next.
//                              Both: slot 0 of a block's partial sums is the full sample (b = -1), slot 1 + b group b; [K][2] = N, X;
//                              a short row contributes to none and raises its flag.
// The short flags become rows by jack_scan_kernel / jack_compact_kernel, the partial sums totals by jack_final_kernel (jack_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "jack_kernels.hpp"
#include "knn_div.hpp"

namespace mce {

constexpr int kDivRegShort = 16;             // lists up to this long stay in registers: the first rung, at half the registers
constexpr int kDivRegL = 32;                 // and up to this long: the second rung
constexpr int kDivNoColumn = 1 << 20;        // "no column" in the minimum over the columns

// par: linv[d][d] then mean[d]; partial: [nblocks][3]
__global__ __launch_bounds__(kRedThreads) void div_whiten_kernel(const double* __restrict__ x, int64_t ld, int64_t n, int d, const double* __restrict__ par,
                                                                 const double* __restrict__ w, double* __restrict__ z, double* __restrict__ partial)
{
    extern __shared__ double div_lds[];          // linv[d * d], mean[d]
    __shared__ double red[kRedWaves];
    for (int i = threadIdx.x; i < d * d + d; i += kRedThreads) div_lds[i] = par[i];
    __syncthreads();
    const double* const linv = div_lds;
    const double* const mean = div_lds + d * d;
    const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    const bool live = i < n;
    double wi = 0.0, bad = 0.0, col = (double)kDivNoColumn;
    if (live) {
        wi = w[i];
        bad = mce_div::div_bad_weight(wi) ? 1.0 : 0.0;
        const double* const xi = x + i * ld;
        for (int k = d - 1; k >= 0; --k)
            if (!mce_div::div_finite(xi[k])) col = (double)k;
        for (int k = 0; k < d; ++k) z[i * (int64_t)d + k] = mce_div::div_whiten_coord(linv + k * d, xi, mean, k);
    }
    const double sw = block_sum(wi, red), sb = block_sum(bad, red), mc = block_min(col, red);
    if (threadIdx.x == 0) {
        partial[(int64_t)blockIdx.x * 3 + 0] = sw;
        partial[(int64_t)blockIdx.x * 3 + 1] = sb;
        partial[(int64_t)blockIdx.x * 3 + 2] = mc;
    }
}

// report: [4] = the sum of w, the bad weights, the lowest non-finite column (-1: none), the rows
__global__ __launch_bounds__(kRedThreads) void div_report_kernel(const double* __restrict__ partial, int64_t nblocks, int64_t n, double* __restrict__ report)
{
    __shared__ double red[kRedWaves];
    double sw = 0.0, sb = 0.0, mc = (double)kDivNoColumn;
    for (int64_t b = threadIdx.x; b < nblocks; b += kRedThreads) {
        sw += partial[b * 3 + 0];
        sb += partial[b * 3 + 1];
        mc = partial[b * 3 + 2] < mc ? partial[b * 3 + 2] : mc;
    }
    sw = block_sum(sw, red);
    sb = block_sum(sb, red);
    mc = block_min(mc, red);
    if (threadIdx.x == 0) {
        report[0] = sw;
        report[1] = sb;
        report[2] = mc >= (double)kDivNoColumn ? -1.0 : mc;
        report[3] = (double)n;
    }
}

// mpart: [nblocks][G + 1]
__global__ __launch_bounds__(kRedThreads) void div_mass_kernel(const double* __restrict__ a, const int32_t* __restrict__ g, int64_t n, int G,
                                                               double* __restrict__ mpart)
{
    __shared__ double red[kRedWaves];
    const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    const bool live = i < n;
    const double ai = live ? a[i] : 0.0;
    const int gi = (live && G > 0) ? g[i] : -1;
    for (int s = 0; s <= G; ++s) {                       // wave-uniform
        const double v = block_sum((s == 0 || gi == s - 1) ? ai : 0.0, red);
        if (threadIdx.x == 0) mpart[(int64_t)blockIdx.x * (G + 1) + s] = v;
    }
}

// the list of one row in registers: the logarithms of the distances, the gathered weights, the group bytes four to a word
template <int RL> struct DivRegList {
    double lr[RL], wt[RL];
    unsigned gw[RL / 4];
};

// partial: [nblocks][G + 1][K][2]; wp: [G + 1] (the weight of P, of its groups); flags: [nq]; block_cnt: [nblocks]
template <int RL>
__global__ __launch_bounds__(kRedThreads) void div_terms_kernel(
    const double* __restrict__ distP, const int64_t* __restrict__ idxP, const double* __restrict__ distQ, const int64_t* __restrict__ idxQ, int64_t nq, int L,
    const int64_t* __restrict__ qid, const int32_t* __restrict__ gq, const int32_t* __restrict__ grP, int64_t nP, const int32_t* __restrict__ grQ, int64_t nQ,
    int G, int K, int D, const double* __restrict__ aq, const double* __restrict__ aP, const double* __restrict__ bQ, const double* __restrict__ wp,
    double* __restrict__ partial, int* __restrict__ flags, int* __restrict__ block_cnt)
{
    using namespace mce_jack;
    using namespace mce_div;
    __shared__ double red[kRedWaves];
    __shared__ int cnt[kRedWaves];
    const int64_t q = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    const bool live = q < nq;
    double ai = 0.0;
    int own = -2;                                        // (no groups: no slot is the row's own)
    int64_t self = -1;
    if (live) {
        ai = aq[q];
        own = G > 0 ? gq[q] : -2;
        self = qid ? qid[q] : q;
    }
    const int64_t* const ia = idxP + (live ? q : 0) * (int64_t)L;
    const int64_t* const ib = idxQ + (live ? q : 0) * (int64_t)L;
    const double* const da = distP + (live ? q : 0) * (int64_t)L;
    const double* const db = distQ + (live ? q : 0) * (int64_t)L;
    auto group_a = [&](int j) { return div_entry_group(ia[j], nP, grP, self); };
    auto group_b = [&](int j) { return div_entry_group(ib[j], nQ, grQ, -1); };

    constexpr bool REG = RL > 0;
    DivRegList<REG ? RL : 4> A, B;
    bool is_short = false;
    if constexpr (REG) {
        int va = 0, vb = 0;
#pragma unroll
        for (int j = 0; j < RL / 4; ++j) A.gw[j] = B.gw[j] = 0xffffffffu;
#pragma unroll
        for (int j = 0; j < RL; ++j) {
            A.lr[j] = B.lr[j] = 0.0;
            A.wt[j] = B.wt[j] = 0.0;
            if (j < L && live) {
                const int ga = group_a(j), gb = group_b(j);
                if (ga != kJackSkip) {
                    A.lr[j] = log(da[j]);
                    A.wt[j] = aP[ia[j]];
                    A.gw[j >> 2] = (A.gw[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((unsigned)ga << (8 * (j & 3)));
                    ++va;
                }
                if (gb != kJackSkip) {
                    B.lr[j] = log(db[j]);
                    B.wt[j] = bQ[ib[j]];
                    B.gw[j >> 2] = (B.gw[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((unsigned)gb << (8 * (j & 3)));
                    ++vb;
                }
            }
        }
        is_short = va < K || vb < K;
        for (int b = 0; b < G; ++b) {
            int na = 0, nb = 0;
#pragma unroll
            for (int j = 0; j < RL; ++j) {
                na += (int)((A.gw[j >> 2] >> (8 * (j & 3))) & 0xffu) == b;
                nb += (int)((B.gw[j >> 2] >> (8 * (j & 3))) & 0xffu) == b;
            }
            if (b != own && (va - na < K || vb - nb < K)) is_short = true;
        }
    } else {
        if (live) is_short = div_is_short(group_a, group_b, L, own, G, K);
    }
    if (!live) is_short = false;

    // the short flag, and how many of them this block holds (integer counts: ballot per wave, then four adds)
    {
        const unsigned long long m = __ballot(is_short);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (live) flags[q] = is_short ? 1 : 0;
        if (lane == 0) cnt[wv] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) {
            int s = 0;
            for (int i = 0; i < kRedWaves; ++i) s += cnt[i];
            block_cnt[blockIdx.x] = s;
        }
    }

    double* const out = partial + (int64_t)blockIdx.x * (G + 1) * K * 2;
    const double wall = wp[0];
    for (int b = -1; b < G; ++b) {                       // wave-uniform
        const bool in = live && !is_short && own != b;
        const double lw = log((b < 0 ? wall : wall - wp[1 + b]) - ai);
        double* const ob = out + (int64_t)(b + 1) * K * 2;
        if constexpr (REG) {
            // the kept entries of either list as a bit mask; rank k is its k-th set bit, found by clearing the lowest bit rank by rank
            unsigned ma = 0u, mb = 0u;
#pragma unroll
            for (int j = 0; j < RL; ++j) {
                ma |= jack_keep((int)((A.gw[j >> 2] >> (8 * (j & 3))) & 0xffu), b) ? 1u << j : 0u;
                mb |= jack_keep((int)((B.gw[j >> 2] >> (8 * (j & 3))) & 0xffu), b) ? 1u << j : 0u;
            }
            double ra = 0.0, rb = 0.0;
            for (int k = 0; k < K; ++k) {                // wave-uniform
                const int pa = __ffs(ma) - 1, pb = __ffs(mb) - 1;          // (-1 where a list ran out: a short row, which is not `in`)
                ma &= ma - 1u;
                mb &= mb - 1u;
                double lrho = 0.0, wa = 0.0, lnu = 0.0, wb = 0.0;
#pragma unroll
                for (int j = 0; j < RL; ++j) {           // compare-and-select: no indexed private array
                    lrho = j == pa ? A.lr[j] : lrho;
                    wa = j == pa ? A.wt[j] : wa;
                    lnu = j == pb ? B.lr[j] : lnu;
                    wb = j == pb ? B.wt[j] : wb;
                }
                ra += wa;
                rb += wb;
                const bool zero = div_coincident(lrho, lnu);
                const double s = div_s(D, lnu, lrho, ra, rb, lw);
                const double sn = block_sum((in && !zero) ? ai * s : 0.0, red);
                const double sx = block_sum((in && zero) ? ai : 0.0, red);
                if (threadIdx.x == 0) {
                    ob[2 * k] = sn;
                    ob[2 * k + 1] = sx;
                }
            }
        } else {
            JackCursor ca, cb;
            double ra = 0.0, rb = 0.0;
            for (int k = 0; k < K; ++k) {
                double tn = 0.0, tx = 0.0;
                if (in) {
                    const int ja = jack_next(group_a, L, b, ca), jb = jack_next(group_b, L, b, cb);
                    if (ja >= 0 && jb >= 0) {          // (always: the row is not short, so neither list runs out; a kept entry's row is in range)
                        ra += aP[ia[ja]];
                        rb += bQ[ib[jb]];
                        const double lrho = log(da[ja]), lnu = log(db[jb]);
                        if (div_coincident(lrho, lnu)) tx = ai;
                        else tn = ai * div_s(D, lnu, lrho, ra, rb, lw);
                    }
                }
                const double sn = block_sum(tn, red), sx = block_sum(tx, red);
                if (threadIdx.x == 0) {
                    ob[2 * k] = sn;
                    ob[2 * k + 1] = sx;
                }
            }
        }
    }
}

}  // namespace mce
