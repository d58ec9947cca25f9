// prune.hpp -- interface of prune.hip: spatial pruning for low-dimensional, large reference sets
// (SURVEY.md section 8f.2(ii)).
//
// The brute-force sweep of knn_f16.hpp visits every (query block, reference chunk) pair.  For
// D <~ 10 and N >~ 10^6 almost all of them are provably irrelevant: if both point sets are laid
// out in k-d order, a block of 512 queries sits in a small box, and a chunk of references whose
// box is farther from it than the block's current worst K-th distance cannot contribute.  This
// module produces, entirely on the device and stream-ordered (no host synchronisation):
//   * a k-d ordering of the references and of the queries down to cells of 32 rows (= one MFMA
//     tile): recursive median splits cycling through the dimensions, implemented as one radix
//     sort per tree level on the key (node id, coordinate);
//   * the reordered fp64 copies Ys / Xs and the permutations back to the caller's row numbers;
//   * the bounding box of every 32-row tile (floats rounded outward);
//   * per query block, the list of ALL reference chunks sorted by box-to-box distance (a rigorous
//     lower bound, rounded down) -- the search kernel walks it, stops at the first entry whose
//     bound exceeds the block's current threshold, and inside a chunk multiplies only the tiles
//     whose box is within reach of one of the wave's two query tiles.
// Results are those of the exhaustive search, bit for bit (same exact distances, same tie-breaks
// on the caller's row numbers).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "search_layout.hpp"      // PruneArena, SymArena: where the arrays below lie

namespace mce {

constexpr int kPruneMaxDim = 15;                          // KST = 1 variants only
constexpr int64_t kPruneMaxPairs = (int64_t)1 << 30;      // nqblk * nchunk list entries

// rocPRIM's temporary storage for the sorts of a k-d preparation: nmax = max(nq_pad, nr_pad) rows, nwaves = nqblk * kPruneWavesPerBlock
// (host-only size query; -> SearchSizes::prune_tmp_bytes)
size_t prune_tmp_bytes(int64_t nmax, size_t nwaves);

// The chunk lists are ordered by BANDS of the lower bound (the float's exponent and its top kPruneBandMantissa mantissa bits:
// 3 % wide), not entry by entry: prune_band_floor(d) <= d is the same for every entry of a band and never decreases along a
// list, so the walk may stop at the first entry whose band floor exceeds its reach (knn_f16.hpp) -- and a counting sort by
// band in one pass replaces a segmented radix sort of nqblk * nchunk pairs.
constexpr int kPruneBandMantissa = 5;
__host__ __device__ inline float prune_band_floor(float d2)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(__float_as_uint(d2) & ~((1u << (23 - kPruneBandMantissa)) - 1u));
#else
    union { float f; unsigned u; } v; v.f = d2; v.u &= ~((1u << (23 - kPruneBandMantissa)) - 1u); return v.f;
#endif
}

// Fills the arena: the k-d ordered copies Ys / Xs, the permutations, the boxes, every block's chunk list and the waves' dispatch order.
// same_set: the queries ARE the reference rows (same pointer, nq == nr): one ordering serves both -- the queries' rows, permutation and
// tile boxes are then the references' (Ys, perm_r, tbox_r; Xs, perm_q and tbox_q stay unwritten)
// perm_ready (round 6): the k-d order of the references is in the workspace already (prune_prepare_part + the ranks' all-reduce)
hipError_t prune_prepare(const double* dX, int64_t nq, const double* dY, int64_t nr, int d, bool same_set, int qpb,
                         int chunk_rows, int64_t nq_pad, int nqblk, int64_t nr_pad, int64_t nchunk, const PruneArena& A,
                         hipStream_t st, bool perm_ready = false);
// Distributed k-d preparation (round 6; reference: the `fit` of MCEvidence.py:1100-1101, which every rank of a multi-GPU run repeated
// in full -- 4.85 ms of sorts of the 7.8 ms a rank of C5 spends preparing): rank `part` of nparts = 2, 4, 8, ... runs the sorts that
// settle the tree's top log2(nparts) levels over all rows and everything below them over ITS subtree only; perm_r then holds the
// final order in [seg_lo, seg_hi) and zeros elsewhere -- the ranks' arrays add up to the single-GPU permutation, bit for bit.
// seg_lo = 0, seg_hi = nr_pad: the whole order was made here (a count that is not a power of two, a tree too shallow).
hipError_t prune_prepare_part(const double* dY, int64_t nr, int d, int64_t nr_pad, const PruneArena& A, int part, int nparts,
                              hipStream_t st, int64_t& seg_lo, int64_t& seg_hi);

// ---- symmetric sweep (knn_f16.hpp, "Symmetric sweep"): rows sorted by distance from the mean + its scratch ----
// rocPRIM's temporary storage for the sort of n_pad rows (host-only size query; -> SearchSizes::sym_tmp_bytes)
size_t sym_tmp_bytes(int64_t n_pad);
// sorts the rows of Y[n, d] by their distance from `center` (device pointer, d doubles), writes the sorted copy and the
// permutation; stream-ordered, no host synchronisation
hipError_t sym_prepare(const double* dY, int64_t n, int d, const double* center, int64_t n_pad, const SymArena& A, hipStream_t st);

}  // namespace mce
