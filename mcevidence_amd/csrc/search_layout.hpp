// search_layout.hpp -- where everything of one nearest-neighbour search lies in its workspace: the k-d preparation of the pruned walk
// (PruneArena), the symmetric sweep's scratch (SymArena), the search itself in its four shapes (SearchArena) and one rank's share of the
// all-pairs-once partition (PairsOnceArena).  Each is a row of WsPlan takes like feed_layout.hpp's: a field's line declares the array,
// gives its element type, places it and says what it holds, in the order of the memory.  The sizes come in as plain numbers
// (SearchSizes: the planner fills them, capi_plan.hpp: plan_sizes); without a base a constructor only sizes (`total`), with one it
// also leaves the typed pointers.  Host only, plain C++17, no device header: tests/native/search_layout_check.cpp compiles it on the
// CPU and pins it to the offsets the planner counted by hand before.  Every array starts on a multiple of 256 bytes.
#pragma once
#include <cstddef>
#include <cstdint>

#include "ws_plan.hpp"

namespace mce {

constexpr int kPruneTileRows = 32;          // k-d cells = MFMA reference tiles = query tiles
constexpr int kPruneWavesPerBlock = 8;      // == kHWaves (knn_f16.hpp): the walk's workgroups serve one wave of a query block each
constexpr size_t kSymEntryBytes = 16;
struct SymEntry;                            // (sym_types.hpp: a row-side candidate, kSymEntryBytes long)
struct half_t { uint16_t bits; };           // an fp16 element of the packed planes, for a host compiler (the kernels read _Float16)

enum class SearchFamily { long_rows, generic, sweep64, filter };

// what a plan needs room for: numbers only
struct SearchSizes {
    SearchFamily family = SearchFamily::filter;
    int64_t nq = 0, nr = 0;                 // rows of the two sets
    int64_t nq_pad = 0, nrow_pad = 0;       // ... padded to whole query blocks / reference chunks
    int64_t nchunk = 0;                     // reference chunks
    int nqblk = 0, d = 0, K = 0;
    int KS = 0, KST = 0, KCAP = 0;          // k-steps of the fp64 sweeps / of the fp16 filter; list capacity
    int list_sets = 1;                      // list sets [KCAP][nq_pad] to allot: reference splits (x 2 passes) or chains of the symmetric sweep
    size_t center_doubles = 0, msum_doubles = 0, params_doubles = 0;    // centre (| boxes), the column statistics' partial sums, the filter's parameter block
    bool prune = false;                     // the pruned walk's k-d preparation (PruneArena)
    size_t prune_tmp_bytes = 0;             // ... rocPRIM's temporary storage for its sorts (prune.hip: prune_tmp_bytes)
    int heavy_max = 0;                      // ... room for this many heavy waves' side lists (0: none), each of
    int heavy_cols = 0;                     // ... this many list columns
    bool sym = false;                       // the symmetric sweep's scratch (SymArena)
    int sym_cap = 0;                        // ... bucket entries per query block
    size_t sym_tmp_bytes = 0;               // ... rocPRIM's temporary storage for its sort (prune.hip: sym_tmp_bytes)
};

// ---- pruned walk (prune.hpp): k-d order of both sets, boxes, chunk lists ----
struct PruneArena {
    SearchSizes z;
    WsPlan P;
    int64_t nmax = z.nq_pad > z.nrow_pad ? z.nq_pad : z.nrow_pad, nbig = z.nq > z.nr ? z.nq : z.nr;
    size_t ntile_r = (size_t)(z.nrow_pad / kPruneTileRows), ntile_q = (size_t)(z.nq_pad / kPruneTileRows);
    size_t nwaves = (size_t)z.nqblk * kPruneWavesPerBlock, pairs = (size_t)z.nqblk * (size_t)z.nchunk;
    int* perm_r = P.take<int>((size_t)z.nrow_pad);                      // sorted position -> caller's row (-1: padding), references
    int* perm_q = P.take<int>((size_t)z.nq_pad);                        // ... queries
    unsigned long long* keys_a = P.take<unsigned long long>((size_t)nmax);              // sort keys (ping-pong; 32-bit keys use their first halves)
    unsigned long long* keys_b = P.take<unsigned long long>((size_t)nmax);
    int* vals_b = P.take<int>((size_t)nmax);
    double* Ys = P.take<double>((size_t)z.nr * z.d);                    // reordered rows [nr][d]
    double* Xs = P.take<double>((size_t)z.nq * z.d);                    // ... [nq][d]
    // float planes [d][n] of the set being sorted (kd_sort): inside Xs where that is large enough (it is written only after the last sort)
    bool cf32_in_Xs = (size_t)z.nq * z.d * sizeof(double) >= (size_t)nbig * z.d * sizeof(float);
    float* cf32 = cf32_in_Xs ? reinterpret_cast<float*>(Xs) : P.take<float>((size_t)nbig * z.d);
    float* tbox_r = P.take<float>(ntile_r * 2 * z.d);                   // tile boxes [tiles][2][d] (lo | hi), rounded outward
    float* tbox_q = P.take<float>(ntile_q * 2 * z.d);
    float* tboxT_r = P.take<float>(ntile_r * 2 * z.d);                  // [nchunk][2][d][tiles per chunk]: the kernel's layout
    float* box_r = P.take<float>((size_t)z.nchunk * 2 * z.d);           // chunk boxes [nchunk][2][d]
    float* box_q = P.take<float>((size_t)z.nqblk * 2 * z.d);            // query-block boxes [nqblk][2][d]
    float* bkey_a = P.take<float>(nwaves);                              // the walk's waves (block * 8 + wave) by descending box size:
    float* bkey_b = P.take<float>(nwaves);                              // ... keys (ping-pong),
    int* bval_a = P.take<int>(nwaves);                                  // ... wave ids,
    int* border = P.take<int>(nwaves);                                  // ... the dispatch order
    float* list_d = P.take<float>(pairs);                               // [nqblk][nchunk] every block's chunks in bands of ascending box distance: bounds,
    int* list_c = P.take<int>(pairs);                                   // ... chunk ids
    char* tmp = P.take_bytes<char>(z.prune_tmp_bytes);                  // rocPRIM scratch
    size_t total = P.total;
    explicit PruneArena(const SearchSizes& sizes = SearchSizes(), void* base = nullptr) : z(sizes), P(base) {}
};

// ---- symmetric sweep (knn_f16.hpp, "Symmetric sweep"): rows sorted by distance from the mean + its scratch ----
struct SymArena {
    SearchSizes z;
    WsPlan P;
    int cap = z.sym_cap;                                                // bucket entries per query block
    int* perm = P.take<int>((size_t)z.nq_pad);                          // sorted position -> caller's row (-1: padding)
    unsigned* keys_a = P.take<unsigned>((size_t)z.nq_pad);              // sort keys (ping-pong)
    unsigned* keys_b = P.take<unsigned>((size_t)z.nq_pad);
    int* vals_a = P.take<int>((size_t)z.nq_pad);
    double* Ys = P.take<double>((size_t)z.nr * z.d);                    // sorted rows [n][d] (queries and references)
    unsigned long long* thr = P.take<unsigned long long>((size_t)z.nq_pad);             // published bounds
    unsigned* rrow = P.take<unsigned>((size_t)z.nq_pad);                // row-side gate constants
    float* rtile = P.take<float>((size_t)(z.nq_pad / 32));              // ... their maxima per tile
    unsigned long long* slots = P.take<unsigned long long>((size_t)z.nq_pad * z.KCAP);  // [n_pad][KCAP]
    int* counters = P.take<int>((size_t)z.nqblk * 3);                   // ONE array, cleared by one memset: bucket_cnt | bucket_flag | done, [nqblk] each
    SymEntry* bucket = P.take_bytes<SymEntry>((size_t)z.nqblk * cap * kSymEntryBytes);  // [nqblk][cap]
    char* tmp = P.take_bytes<char>(z.sym_tmp_bytes);                    // rocPRIM scratch
    size_t total = P.total;
    explicit SymArena(const SearchSizes& sizes = SearchSizes(), void* base = nullptr) : z(sizes), P(base) {}
    int* bucket_cnt() const { return counters; }
    int* bucket_flag() const { return counters ? counters + z.nqblk : nullptr; }
    int* done() const { return counters ? counters + 2 * (size_t)z.nqblk : nullptr; }
    size_t counters_bytes() const { return (size_t)z.nqblk * 3 * sizeof(int); }
};

struct ListSets { double* d; int* i; };     // list sets [sets][KCAP][nq_pad]: distances, rows

// ---- one search: four shapes, by family.  A line places its array in the shapes named on it; top to bottom is the order of the memory:
//   long rows   pd | pi | center | msum | yfl | xf | xn | slack
//   generic     pd | pi | dist | slack
//   fp64 sweep  yf | pd | pi | center | msum
//   filter      yh | xh | qinfo | params | pd | pi | center | msum | [prune | heavy] | [sym]
struct SearchArena {
    SearchSizes z;
    WsPlan P;
    bool lng = z.family == SearchFamily::long_rows, gen = z.family == SearchFamily::generic, s64 = z.family == SearchFamily::sweep64, flt = z.family == SearchFamily::filter;
    size_t list_entries = (size_t)z.list_sets * z.KCAP * (size_t)z.nq_pad, heavy_entries = (size_t)z.heavy_max * z.heavy_cols * z.KCAP;
    half_t* yh = flt ? P.take<half_t>((size_t)z.nrow_pad * 16 * z.KST) : nullptr;           // filter: the references as fp16 planes [nrow_pad][16 KST],
    half_t* xh = flt ? P.take<half_t>((size_t)z.nq_pad * 16 * z.KST) : nullptr;             // ... the queries [nq_pad][16 KST],
    double* qinfo = flt ? P.take<double>((size_t)z.nq_pad * 2) : nullptr;                   // ... two constants per query,
    double* params = flt ? P.take<double>(z.params_doubles) : nullptr;                      // ... the parameter block
    double* yf = s64 ? P.take<double>((size_t)z.nrow_pad * z.KS * 4) : nullptr;             // fp64 sweep: the references in MFMA fragment order [nrow_pad][4 KS]
    double* pd = P.take<double>(list_entries);                                              // the lists [list_sets][KCAP][nq_pad]: distances,
    int* pi = P.take<int>(list_entries);                                                    // ... rows
    double* center = gen ? nullptr : P.take<double>(z.center_doubles);                      // centre (| box(Y) | box(X))
    double* msum = gen ? nullptr : P.take<double>(z.msum_doubles);                          // partial sums of the column statistics
    double* yfl = lng ? P.take<double>((size_t)z.nrow_pad * z.KS * 4) : nullptr;            // long rows: the references in fragment order [nrow_pad][4 KS],
    double* xf = lng ? P.take<double>((size_t)z.nq_pad * z.KS * 4) : nullptr;               // ... the queries [nq_pad][4 KS]
    double* xn = lng ? P.take<double>((size_t)z.nq_pad) : nullptr;                          // ... and their squared norms
    double* dist = gen ? P.take<double>((size_t)z.nq * z.K) : nullptr;                      // generic: the distance matrix [nq][K] of the fused path
    char* slack = lng || gen ? P.take_bytes<char>(256) : nullptr;                           // long rows, generic: 256 bytes these plans have always ended with (never read)
    PruneArena prune = flt && z.prune ? PruneArena(z, P.here()) : PruneArena();             // filter, pruned walk: a row of its own,
    char* prune_block = P.take_bytes<char>(flt && z.prune ? prune.total : 0);               // ... (its bytes in this row; read through `prune`)
    double* heavy_d = flt && z.prune && z.heavy_max > 0 ? P.take_bytes<double>(heavy_entries * (sizeof(double) + sizeof(int))) : nullptr;   // ... ONE array: the heavy waves' side lists, distances | rows
    SymArena sym = flt && z.sym ? SymArena(z, P.here()) : SymArena();                       // filter, symmetric sweep: a row of its own
    char* sym_block = P.take_bytes<char>(flt && z.sym ? sym.total : 0);                     // ... (its bytes in this row; read through `sym`)
    size_t total = P.total;
    explicit SearchArena(const SearchSizes& sizes = SearchSizes(), void* base = nullptr) : z(sizes), P(base) {}
    int* heavy_i() const { return heavy_d ? reinterpret_cast<int*>(heavy_d + heavy_entries) : nullptr; }
    ListSets lists() const { return ListSets{pd, pi}; }
};

// ---- one rank's share of the all-pairs-once partition (capi_apo.hpp): search | partial | [S list sets] ----
struct PairsOnceArena {
    SearchArena A;
    WsPlan P;
    int S;                                                              // chains per block, each with a list set of its own
    size_t dotp_bytes;
    char* search = P.take_bytes<char>(A.total);                         // the symmetric sweep's arena: its bytes in this row, read through A
    double* partial = P.take_bytes<double>(dotp_bytes);                 // the reduction's partial sums
    double* sets_d = S > 1 ? P.take<double>(set_entries()) : nullptr;   // S > 1: [S][KCAP][nq_pad] distances,
    int* sets_i = S > 1 ? P.take<int>(set_entries()) : nullptr;         // ... rows
    size_t total = P.total;
    PairsOnceArena(const SearchSizes& sizes, size_t dotp_bytes_, int S_, void* base = nullptr) : A(sizes, base), P(base), S(S_), dotp_bytes(dotp_bytes_) {}
    size_t set_entries() const { return (size_t)S * A.z.KCAP * (size_t)A.z.nq_pad; }
    ListSets lists() const { return S > 1 ? ListSets{sets_d, sets_i} : A.lists(); }     // its own sets, or the plan's
};

}  // namespace mce
