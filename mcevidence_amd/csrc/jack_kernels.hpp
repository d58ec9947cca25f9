// jack_kernels.hpp -- the delete-a-group jackknife sums on the device (rule: jack.hpp; docs/design/jackknife.md).  fp64 throughout, plain
// stores, no floating-point atomics: every sum is a block_sum over 256 rows followed by a fixed-order pass over the blocks, so the
// order of every addition is fixed by the sizes alone.
//
//   jack_check_groups_kernel   a group id outside [0, G) raises a flag (the host refuses the call)
//   jack_partial_kernel<REG>   one lane per query, 256 queries per workgroup.  REG (L <= kJackRegL): the list's group bytes and terms
//                              are formed once and kept in registers; the loop over the deleted group b is wave-uniform and picks the
//                              K kept terms by compare-and-select (no indexed private array).  !REG (longer lists, the few rows of the
//                              ladder's upper rungs): the list is walked from memory per group with jack_next, terms formed for the kept
//                              entries only.  Both: slot 0 of a block's partial sums is the full sample (b = -1), slot 1 + b group b;
//                              a short row contributes to none and raises its flag.
//   jack_final_kernel          block (slot, k) sums partial[:, slot, k] in dotp_final_kernel's order
//   jack_scan_kernel, jack_compact_kernel    the short flags -> their rows, ascending: per-block counts, an integer exclusive prefix
//                              sum over the blocks by one workgroup, ranks inside a block by ballot
// With no short row, slot 0 repeats dotp_partial_kernel / dotp_final_kernel on the same distances addition by addition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_reduce.hpp"
#include "jack.hpp"

namespace mce {

constexpr int kJackRegL = 32;      // lists up to this long stay in registers

__global__ __launch_bounds__(kRedThreads) void jack_check_groups_kernel(const int32_t* __restrict__ g, int64_t n, int G, int* __restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    if (i < n && (g[i] < 0 || g[i] >= G)) *bad = 1;
}

// partial: [nblocks][G + 1][kmax]; flags: [nq]; block_cnt: [nblocks]
template <bool REG>
__global__ __launch_bounds__(kRedThreads) void jack_partial_kernel(
    const double* __restrict__ dist, const int64_t* __restrict__ idx, int64_t nq, int L, const int64_t* __restrict__ qid,
    const int32_t* __restrict__ gq, const int32_t* __restrict__ gr, int64_t nr, int G, int k0, int kmax, int D, double lnc,
    const double* __restrict__ w, const double* __restrict__ fs, double* __restrict__ partial, int* __restrict__ flags,
    int* __restrict__ block_cnt)
{
    using namespace mce_jack;
    __shared__ double red[kRedThreads / 64];
    __shared__ int cnt[kRedThreads / 64];
    const int64_t q = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    const bool live = q < nq;
    const int K = kmax - k0;
    double base = 0.0, sgn = 1.0;
    int own = -1;
    int64_t self = -1;
    if (live) {
        const double wq = w[q];
        base = lnc - log(fabs(wq)) + fs[q];
        sgn = wq < 0.0 ? -1.0 : 1.0;
        own = gq[q];
        if (k0 == 1) self = qid ? qid[q] : q;
    }
    const int64_t* const li = idx + (live ? q : 0) * (int64_t)L;
    const double* const ld = dist + (live ? q : 0) * (int64_t)L;

    int g[REG ? kJackRegL : 1];
    double term[REG ? kJackRegL : 1];
    bool is_short = false;
    if constexpr (REG) {
        int valid = 0;
#pragma unroll
        for (int j = 0; j < kJackRegL; ++j) {
            g[j] = kJackSkip;
            term[j] = 0.0;
            if (j < L && live) {
                g[j] = jack_entry_group(li[j], nr, gr, self);
                const double r = ld[j];
                term[j] = sgn * exp(base + (double)D * log(r));
                valid += g[j] != kJackSkip;
            }
        }
        is_short = valid < K;
        for (int b = 0; b < G; ++b) {
            int inb = 0;
#pragma unroll
            for (int j = 0; j < kJackRegL; ++j) inb += g[j] == b;
            if (b != own && valid - inb < K) is_short = true;
        }
    } else {
        if (live)
            is_short = jack_is_short([&](int j) { return jack_entry_group(li[j], nr, gr, self); }, L, own, G, K);
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
            for (int i = 0; i < kRedThreads / 64; ++i) s += cnt[i];
            block_cnt[blockIdx.x] = s;
        }
    }

    double* const out = partial + (int64_t)blockIdx.x * (G + 1) * kmax;
    for (int b = -1; b < G; ++b) {                       // wave-uniform
        const bool in = live && !is_short && own != b;
        double t[kJackMaxK];
#pragma unroll
        for (int k = 0; k < kJackMaxK; ++k) t[k] = 0.0;
        if constexpr (REG) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < kJackRegL; ++j) {
                const bool keep = jack_keep(g[j], b);
#pragma unroll
                for (int k = 0; k < kJackMaxK; ++k)
                    if (k <= j) t[k] = (keep && c == k) ? term[j] : t[k];
                c += keep ? 1 : 0;
            }
        } else if (in) {
            JackCursor c;
            auto group_at = [&](int j) { return jack_entry_group(li[j], nr, gr, self); };
            for (int k = 0; k < K; ++k) {
                const int at = jack_next(group_at, L, b, c);
                const double v = sgn * exp(base + (double)D * log(ld[at < 0 ? 0 : at]));
#pragma unroll
                for (int kk = 0; kk < kJackMaxK; ++kk)
                    if (kk == k) t[kk] = v;
            }
        }
#pragma unroll
        for (int kk = 0; kk < kJackMaxK; ++kk) {
            if (kk < K) {
                const double s = block_sum(in ? t[kk] : 0.0, red);
                if (threadIdx.x == 0) out[(int64_t)(b + 1) * kmax + k0 + kk] = s;
            }
        }
    }
}

// block (slot, k): full[k] (slot 0) or groups[(slot - 1) * kmax + k] = sum over the blocks of partial[blk][slot][k], in dotp_final_kernel's order
__global__ __launch_bounds__(kRedThreads) void jack_final_kernel(const double* __restrict__ partial, int64_t nblocks, int nslots, int k0, int kmax,
                                                                 double* __restrict__ full, double* __restrict__ groups)
{
    __shared__ double red[kRedThreads / 64];
    const int slot = blockIdx.x / kmax, k = blockIdx.x % kmax;
    double* const out = slot == 0 ? full : groups + (int64_t)(slot - 1) * kmax;
    if (k < k0) {
        if (threadIdx.x == 0) out[k] = 0.0;
        return;
    }
    double acc = 0.0;
    for (int64_t b = threadIdx.x; b < nblocks; b += kRedThreads) acc += partial[(b * nslots + slot) * kmax + k];
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) out[k] = s;
}

// one workgroup: block_off[i] = block_cnt[0] + .. + block_cnt[i - 1]; *total = the sum of all
__global__ __launch_bounds__(kRedThreads) void jack_scan_kernel(const int* __restrict__ block_cnt, int64_t nblocks, int64_t* __restrict__ block_off,
                                                                int64_t* __restrict__ total)
{
    __shared__ int64_t seg[kRedThreads];
    const int64_t per = (nblocks + kRedThreads - 1) / kRedThreads;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += block_cnt[i];
    seg[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int i = 0; i < kRedThreads; ++i) {
            const int64_t v = seg[i];
            seg[i] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    int64_t run = seg[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        block_off[i] = run;
        run += block_cnt[i];
    }
}

// short_rows[block_off[block] + rank of the row among the block's flagged rows] = the row (its qid, where given)
__global__ __launch_bounds__(kRedThreads) void jack_compact_kernel(const int* __restrict__ flags, int64_t nq, const int64_t* __restrict__ qid,
                                                                   const int64_t* __restrict__ block_off, int64_t* __restrict__ short_rows)
{
    __shared__ int cnt[kRedThreads / 64];
    const int64_t q = (int64_t)blockIdx.x * kRedThreads + threadIdx.x;
    const bool f = q < nq && flags[q] != 0;
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) cnt[wv] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    for (int i = 0; i < wv; ++i) before += cnt[i];
    if (f) short_rows[block_off[blockIdx.x] + before] = qid ? qid[q] : q;
}

}  // namespace mce
