// chain_farm_kernels.hpp -- the segmented passes of a wave of chain files (capi_farm.hpp; rules in chain_farm.hpp).
//
// The tile passes and scans of chain_kernels.hpp run once over the whole wave; what is per FILE or per ROOT is here:
//   farm_pad_kernel        '\n' into every gap of the layout (one block per file): a file boundary becomes the end of a file
//   farm_files_kernel      per file: first token, tokens, columns, rows, "tokens no multiple of the columns" (one thread per file)
//   farm_rows_kernel       one lane per token; the lane of a row's first token applies the ragged rule inside its file
// and the preparation of the roots of a wave that are not thinned (a root: a list of parts, chain_farm.hpp's row table):
//   farm_gather_kernel     one lane per (row, column) of every root: the packed parameter rows, w and the likelihood column
//   farm_like_tile_kernel  prep_like_tile per 512-row tile IN THE ROOT'S OWN ROW NUMBERING (a tile never spans two roots)
//   farm_like_final_kernel prep_like_final, one block per root
//   farm_fs_kernel         fs = logL - max(logL) of the row's root
// The reductions ARE those of chain_prep_kernels.hpp (prep_like_tile, prep_like_final, prep_logl, called with the root as the
// segment), so a root's bits depend on its own rows only and equal what mce_chain_reduce_dev gives the root alone.
// No floating-point atomics, plain C++ stores, 64-bit indices; a row the table cannot place writes NaN and reads nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "chain_farm.hpp"
#include "chain_kernels.hpp"
#include "chain_prep_kernels.hpp"

namespace mce {

static_assert(mce_farm::kTileBytes == kChainTileBytes, "one tile size");

__global__ __launch_bounds__(kChainThreads) void farm_pad_kernel(unsigned char* __restrict__ text, const int64_t* __restrict__ file_off,
                                                                const int64_t* __restrict__ file_len, int64_t nfiles, int64_t wave_bytes)
{
    for (int64_t f = blockIdx.x; f < nfiles; f += gridDim.x) {
        const int64_t lo = file_off[f] + file_len[f], hi = f + 1 < nfiles ? file_off[f + 1] : wave_bytes;
        for (int64_t i = lo + threadIdx.x; i < hi && i < wave_bytes; i += kChainThreads)
            if (i >= 0) text[i] = (unsigned char)mce_farm::kPadByte;
    }
}

// file_tile0[nfiles + 1] (the last entry: ntiles); tile_tok_base: chain_scan_count_kernel's exclusive sums
__global__ __launch_bounds__(kChainThreads) void farm_files_kernel(const int64_t* __restrict__ tok_line, const int64_t* __restrict__ file_tile0, int64_t nfiles,
                                                                  const unsigned long long* __restrict__ tile_tok_base, int64_t ntiles,
                                                                  const ChainTotals* __restrict__ tot, mce_farm::FileVerdict* __restrict__ files,
                                                                  int64_t* __restrict__ file_tok0)
{
    const int64_t ntok = (int64_t)tot->ntok;
    for (int64_t f = (int64_t)blockIdx.x * kChainThreads + threadIdx.x; f <= nfiles; f += (int64_t)gridDim.x * kChainThreads) {
        const int64_t a = file_tile0[f];
        const int64_t t0 = (f < nfiles && a >= 0 && a < ntiles) ? (int64_t)tile_tok_base[a] : ntok;
        file_tok0[f] = t0;
        if (f == nfiles) continue;
        const int64_t b = file_tile0[f + 1];
        const int64_t t1 = (f + 1 < nfiles && b >= 0 && b < ntiles) ? (int64_t)tile_tok_base[b] : ntok;
        mce_farm::FileVerdict v;
        mce_farm::file_counts(tok_line, t0, t1 < t0 ? t0 : t1, &v);
        files[f] = v;
    }
}

__global__ __launch_bounds__(kChainThreads) void farm_rows_kernel(const int64_t* __restrict__ tok_line, int64_t ntok, const int64_t* __restrict__ file_tok0,
                                                                 int64_t nfiles, mce_farm::FileVerdict* __restrict__ files)
{
    for (int64_t k = (int64_t)blockIdx.x * kChainThreads + threadIdx.x; k < ntok; k += (int64_t)gridDim.x * kChainThreads) {
        const int64_t f = mce_farm::file_of_token(file_tok0, nfiles, k);
        const int64_t t0 = files[f].tok0, ncols = files[f].ncols, n = files[f].ntok;
        if (ncols < 1 || k < t0) continue;
        const int64_t in = k - t0;
        if (in % ncols != 0 || in + ncols > n) continue;          // (not a row's first token / the incomplete last group: ntok % ncols says so)
        if (mce_farm::row_ragged(tok_line, t0, ncols, in / ncols)) files[f].ragged = 1;
    }
}

// ---- preparation, segmented over the roots of a wave ------------------------------------------------------------------------------
// tables (device, int64): row0[nroots + 1], tile0[nroots + 1], part0[nroots + 1], ncols[nroots], elem0[nroots + 1] (prefix sums of
// rows * ncols), param0[nroots + 1] (prefix sums of rows * (ncols - itheta)); parts: part_first[nparts], part_rows[nparts] and
// part_ptr[nparts] (the address of the part's first kept row)
struct FarmTables {
    const int64_t *row0, *tile0, *part0, *ncols, *elem0, *param0, *part_first, *part_rows;
    const double* const* part_ptr;
    int64_t nroots, nparts;
};

__device__ __forceinline__ const double* farm_row(const FarmTables& t, int64_t root, int64_t in_root)
{
    const int64_t pa = t.part0[root], np = t.part0[root + 1] - pa;
    if (np < 1) return nullptr;
    const int64_t p = pa + mce_farm::part_of_row(t.part_first + pa, np, in_root);
    const int64_t local = in_root - t.part_first[p];
    if (local < 0 || local >= t.part_rows[p]) return nullptr;
    return t.part_ptr[p] + local * t.ncols[root];
}

__global__ __launch_bounds__(kPrepThreads) void farm_gather_kernel(FarmTables t, int iw, int ilike, int itheta, double* __restrict__ params,
                                                                  double* __restrict__ w_out, double* __restrict__ like_out)
{
    const int64_t total = t.elem0[t.nroots];
    for (int64_t e = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kPrepThreads) {
        const int64_t root = mce_farm::last_at_or_below(t.elem0, t.nroots, e);
        const int64_t ncols = t.ncols[root], in = e - t.elem0[root];
        const int64_t r = in / ncols;
        const int col = (int)(in - r * ncols);
        const double* row = farm_row(t, root, r);
        const double v = row ? row[col] : __builtin_nan("");
        const int64_t g = t.row0[root] + r;
        if (col >= itheta) params[t.param0[root] + r * (ncols - itheta) + (col - itheta)] = v;
        if (col == iw) w_out[g] = v;
        if (col == ilike) like_out[g] = v;
    }
}

__global__ __launch_bounds__(kPrepThreads) void farm_like_tile_kernel(FarmTables t, const double* __restrict__ like, const double* __restrict__ w, int pos_lnp,
                                                                     double* __restrict__ tile_max, double* __restrict__ tile_sumw,
                                                                     long long* __restrict__ tile_bad)
{
    __shared__ PrepLikeShared s;
    const int64_t ntiles = t.tile0[t.nroots];
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {          // (the same trips for every thread of the block: the barriers inside)
        const int64_t root = mce_farm::last_at_or_below(t.tile0, t.nroots, tile), base = t.row0[root];
        prep_like_tile(s, like + base, w + base, t.row0[root + 1] - base, tile - t.tile0[root], pos_lnp, tile_max + tile, tile_sumw + tile, tile_bad + tile);
    }
}

// out[4 * root ..]: max(logL), SumW, NaN likelihoods, weights that are not finite; one block per root
__global__ __launch_bounds__(kPrepThreads) void farm_like_final_kernel(FarmTables t, const double* __restrict__ tile_max, const double* __restrict__ tile_sumw,
                                                                      const long long* __restrict__ tile_bad, double* __restrict__ out)
{
    __shared__ PrepLikeShared s;
    for (int64_t root = blockIdx.x; root < t.nroots; root += gridDim.x) {
        const int64_t b = t.tile0[root];
        prep_like_final(s, tile_max + b, tile_sumw + b, tile_bad + b, t.tile0[root + 1] - b, out + 4 * root);
        __syncthreads();          // (s is free for the next root)
    }
}

__global__ __launch_bounds__(kPrepThreads) void farm_fs_kernel(FarmTables t, const double* __restrict__ like, int pos_lnp, const double* __restrict__ red,
                                                              double* __restrict__ fs)
{
    const int64_t n = t.row0[t.nroots];
    for (int64_t g = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; g < n; g += (int64_t)gridDim.x * kPrepThreads)
        fs[g] = prep_logl(like[g], pos_lnp) - red[4 * mce_farm::last_at_or_below(t.row0, t.nroots, g)];
}

}  // namespace mce
