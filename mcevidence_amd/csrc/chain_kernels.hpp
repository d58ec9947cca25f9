// chain_kernels.hpp -- chain text -> fp64 on the device (mce_chain_dev_*, capi_chain.hpp): the structure pass and the parse pass.
//
// Semantics are the host reader's (include/mcechains.h): fields separated by ' ', \t, \v, \f; '#' starts a comment that runs to the
// end of the line, glued to a token or not; \n and \r both end a line; every data line has the column count of the first.
//
// The text is cut into tiles of kChainTileBytes (256 threads x 16 bytes, one aligned 16-byte load each).  The buffer is padded to a
// whole number of tiles with '\n', so every tile is read in full and every token ends inside the buffer.
//   1. chain_tile_kernel<0>   per tile: the last '#' or line end in it -- the tile's element of the two-state "inside a comment"
//                             monoid (identity / leaves outside / leaves inside): ONE byte per tile.
//   2. chain_scan_state_kernel   exclusive scan of those: the state in which each tile starts.
//   3. chain_tile_kernel<1>   per tile: token starts and line ends in it (two 32-bit counts).
//   4. chain_scan_count_kernel   exclusive 64-bit sums of the counts, and the totals.
//   5. chain_tile_kernel<2>   writes for token k its byte offset and its line number (line ends before it).
//   6. chain_ncols_kernel, chain_rows_kernel   the per-file verdict of chain_farm.hpp (file_counts, row_ragged) for the one file that
//                             starts at token 0: columns = tokens on the first token's line; every group of ncols consecutive tokens
//                             lies on ONE line and the next group on ANOTHER -- exactly "every line holds 0 or ncols tokens", and
//                             then token k is row k / ncols, column k % ncols.
//   7. chain_parse_kernel     one lane per token (neighbouring lanes read neighbouring bytes): chain_parse.hpp's exact paths;
//                             what they cannot decide goes to a list (token, offset, length) that the host patches with strtod.
// A token starts at a byte outside any comment that is neither space nor line end nor '#' and whose predecessor is a space, a line
// end or the start of the text (a predecessor inside a comment that is not a line end would put the byte inside the comment too).
// All offsets and counts are 64-bit; every loop is bounded by the tile or by kChainMaxToken; plain C++ stores only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_farm.hpp"
#include "chain_parse.hpp"

namespace mce {

constexpr int kChainThreads = 256;
constexpr int kChainBytesPerThread = 16;
constexpr int64_t kChainTileBytes = (int64_t)kChainThreads * kChainBytesPerThread;
constexpr int kChainMaxToken = 4096;          // longer tokens are left to the host, which rejects them (chain_parse.hpp: kMaxTokenBytes)
constexpr int kChainScanThreads = 1024;

// totals and verdicts of one file, in device memory
struct ChainTotals {
    unsigned long long ntok, nterm, ncols, ragged, nlist;
};

// one token the device could not decide
struct ChainPatch {
    int64_t token, offset, length;
};

// (the byte classes and chain_byte_class are chain_farm.hpp's, which the host check compiles too)

// comment-state elements: 0 identity, 1 "ends outside a comment" (a line end came last), 2 "ends inside" ('#' came last);
// a then b = b unless b is the identity
__device__ __forceinline__ int chain_state_of_wave(int kind, int lane, int* before)
{
    const unsigned long long hm = __ballot(kind == 2), tm = __ballot(kind == 1);
    const unsigned long long lower = lane ? (~0ull >> (64 - lane)) : 0ull;
    const unsigned long long h = hm & lower, t = tm & lower;
    *before = (h | t) == 0 ? 0 : (h > t ? 2 : 1);          // (disjoint masks: the larger one holds the highest lane)
    return (hm | tm) == 0 ? 0 : (hm > tm ? 2 : 1);
}

// PHASE 0: tile_kind[tile].  PHASE 1: tile_ntok / tile_nterm, given tile_in.  PHASE 2: tok_off / tok_line, given the bases.
template <int PHASE>
__global__ __launch_bounds__(kChainThreads) void chain_tile_kernel(const unsigned char* __restrict__ text, int64_t ntiles, unsigned char* __restrict__ tile_kind,
                                                                   const unsigned char* __restrict__ tile_in, unsigned* __restrict__ tile_ntok,
                                                                   unsigned* __restrict__ tile_nterm, const unsigned long long* __restrict__ tok_base,
                                                                   const unsigned long long* __restrict__ term_base, int64_t* __restrict__ tok_off,
                                                                   int64_t* __restrict__ tok_line)
{
    __shared__ int s_kind[kChainThreads / 64];
    __shared__ unsigned s_cnt[kChainThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * kChainTileBytes + (int64_t)tid * kChainBytesPerThread;
        const uint4 q = *reinterpret_cast<const uint4*>(text + base);
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        int cls[kChainBytesPerThread];
        int kind = 0;
#pragma unroll
        for (int i = 0; i < kChainBytesPerThread; ++i) {
            cls[i] = chain_byte_class((w[i >> 2] >> (8 * (i & 3))) & 0xFFu);
            if (cls[i] == kByteTerm) kind = 1;
            else if (cls[i] == kByteHash) kind = 2;
        }
        int before = 0;
        const int wkind = chain_state_of_wave(kind, lane, &before);
        if (lane == 0) s_kind[wave] = wkind;
        __syncthreads();
        if (PHASE == 0) {
            if (tid == 0) {
                int k = 0;
                for (int v = 0; v < kChainThreads / 64; ++v)
                    if (s_kind[v]) k = s_kind[v];
                tile_kind[tile] = (unsigned char)k;
            }
            __syncthreads();
            continue;
        }
        for (int v = wave - 1; v >= 0 && before == 0; --v) before = s_kind[v];
        bool in_comment = before ? before == 2 : tile_in[tile] != 0;
        // the class of the byte before this thread's first one
        int prev = kByteTerm;
        if (base > 0) prev = chain_byte_class(text[base - 1]);
        unsigned ntok = 0, nterm = 0, start_mask = 0, term_mask = 0;
#pragma unroll
        for (int i = 0; i < kChainBytesPerThread; ++i) {
            const int c = cls[i];
            if (c == kByteTerm) { in_comment = false; ++nterm; term_mask |= 1u << i; }
            else if (c == kByteHash) in_comment = true;
            else if (c == kByteOther && !in_comment && (prev == kByteSpace || prev == kByteTerm)) { ++ntok; start_mask |= 1u << i; }
            prev = c;
        }
        // exclusive scan of (ntok << 16 | nterm) over the block: at most 4096 of each per tile
        const unsigned mine = (ntok << 16) | nterm;
        unsigned incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) s_cnt[wave] = incl;
        __syncthreads();
        unsigned excl = incl - mine, total = 0;
        for (int v = 0; v < kChainThreads / 64; ++v) {
            if (v < wave) excl += s_cnt[v];
            total += s_cnt[v];
        }
        if (PHASE == 1) {
            if (tid == 0) {
                tile_ntok[tile] = total >> 16;
                tile_nterm[tile] = total & 0xFFFFu;
            }
        } else {
            int64_t k = (int64_t)tok_base[tile] + (excl >> 16);
            int64_t line = (int64_t)term_base[tile] + (excl & 0xFFFFu);
#pragma unroll
            for (int i = 0; i < kChainBytesPerThread; ++i) {
                if (start_mask & (1u << i)) {
                    tok_off[k] = base + i;
                    tok_line[k] = line;
                    ++k;
                }
                if (term_mask & (1u << i)) ++line;
            }
        }
        __syncthreads();
    }
}

// tile_in[t] = 1 if tile t starts inside a comment.  One block; each thread takes a contiguous run of tiles.
__global__ __launch_bounds__(kChainScanThreads) void chain_scan_state_kernel(const unsigned char* __restrict__ tile_kind, int64_t ntiles, unsigned char* __restrict__ tile_in)
{
    __shared__ unsigned char s[kChainScanThreads];
    const int tid = threadIdx.x;
    const int64_t per = (ntiles + kChainScanThreads - 1) / kChainScanThreads;
    const int64_t t0 = min((int64_t)tid * per, ntiles), t1 = min(t0 + per, ntiles);
    int k = 0;
    for (int64_t t = t0; t < t1; ++t)
        if (tile_kind[t]) k = tile_kind[t];
    s[tid] = (unsigned char)k;
    __syncthreads();
    int state = 0;
    for (int v = tid - 1; v >= 0 && state == 0; --v) state = s[v];
    for (int64_t t = t0; t < t1; ++t) {
        tile_in[t] = state == 2 ? 1 : 0;
        if (tile_kind[t]) state = tile_kind[t];
    }
}

// exclusive 64-bit sums of the per-tile counts; totals -> tot->ntok, tot->nterm
__global__ __launch_bounds__(kChainScanThreads) void chain_scan_count_kernel(const unsigned* __restrict__ tile_ntok, const unsigned* __restrict__ tile_nterm, int64_t ntiles,
                                                                             unsigned long long* __restrict__ tok_base, unsigned long long* __restrict__ term_base,
                                                                             ChainTotals* __restrict__ tot)
{
    __shared__ unsigned long long s_a[kChainScanThreads], s_b[kChainScanThreads];
    const int tid = threadIdx.x;
    const int64_t per = (ntiles + kChainScanThreads - 1) / kChainScanThreads;
    const int64_t t0 = min((int64_t)tid * per, ntiles), t1 = min(t0 + per, ntiles);
    unsigned long long a = 0, b = 0;
    for (int64_t t = t0; t < t1; ++t) {
        a += tile_ntok[t];
        b += tile_nterm[t];
    }
    s_a[tid] = a;
    s_b[tid] = b;
    __syncthreads();
    for (int off = 1; off < kChainScanThreads; off <<= 1) {          // inclusive scan in LDS
        unsigned long long ua = 0, ub = 0;
        if (tid >= off) { ua = s_a[tid - off]; ub = s_b[tid - off]; }
        __syncthreads();
        s_a[tid] += ua;
        s_b[tid] += ub;
        __syncthreads();
    }
    unsigned long long ea = s_a[tid] - a, eb = s_b[tid] - b;
    for (int64_t t = t0; t < t1; ++t) {
        tok_base[t] = ea;
        term_base[t] = eb;
        ea += tile_ntok[t];
        eb += tile_nterm[t];
    }
    if (tid == kChainScanThreads - 1) {
        tot->ntok = s_a[tid];
        tot->nterm = s_b[tid];
    }
}

// the verdict of the one file that is the whole text: mce_farm::file_counts over all tokens ...
__global__ void chain_ncols_kernel(const int64_t* __restrict__ tok_line, ChainTotals* __restrict__ tot)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    mce_farm::FileVerdict v;
    mce_farm::file_counts(tok_line, 0, (int64_t)tot->ntok, &v);
    tot->ncols = (unsigned long long)v.ncols;
    tot->ragged = (unsigned long long)v.ragged;
}

// ... and mce_farm::row_ragged, one thread per group of ncols tokens
__global__ __launch_bounds__(kChainThreads) void chain_rows_kernel(const int64_t* __restrict__ tok_line, ChainTotals* __restrict__ tot)
{
    const int64_t ncols = (int64_t)tot->ncols, ntok = (int64_t)tot->ntok;
    if (ncols < 1) return;
    const int64_t nrows = ntok / ncols;
    for (int64_t r = (int64_t)blockIdx.x * kChainThreads + threadIdx.x; r < nrows; r += (int64_t)gridDim.x * kChainThreads)
        if (mce_farm::row_ragged(tok_line, 0, ncols, r)) tot->ragged = 1ull;
}

__global__ __launch_bounds__(kChainThreads) void chain_parse_kernel(const char* __restrict__ text, int64_t nbytes, const int64_t* __restrict__ tok_off, int64_t ntok,
                                                                    const uint64_t* __restrict__ pow5, double* __restrict__ out, ChainPatch* __restrict__ list,
                                                                    int64_t list_cap, ChainTotals* __restrict__ tot)
{
    for (int64_t k = (int64_t)blockIdx.x * kChainThreads + threadIdx.x; k < ntok; k += (int64_t)gridDim.x * kChainThreads) {
        const int64_t o = tok_off[k];
        if (o < 0 || o >= nbytes) continue;          // (cannot happen: offsets come from the structure pass over the same bytes)
        int len = 0;
        while (len <= kChainMaxToken && o + len < nbytes && chain_byte_class((unsigned char)text[o + len]) == kByteOther) ++len;
        double v = 0.0;
        const int rc = len <= kChainMaxToken ? mce_parse::parse_token_exact(text + o, text + o + len, pow5, &v) : mce_parse::kUndecided;
        if (rc == mce_parse::kConverted) out[k] = v;
        else {
            const unsigned long long slot = atomicAdd(&tot->nlist, 1ull);
            if ((int64_t)slot < list_cap) {
                list[slot].token = k;
                list[slot].offset = o;
                list[slot].length = len;
            }
        }
    }
}

}  // namespace mce
