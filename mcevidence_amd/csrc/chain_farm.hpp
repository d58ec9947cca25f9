// chain_farm.hpp -- the rules of a WAVE of chain files parsed in one pass (capi_farm.hpp, chain_farm_kernels.hpp), shared by the host
// check (tests/native/chain_farm_check.cpp, plain C++17 under g++) and the device kernels (__host__ __device__ under hipcc), after the
// pattern of chain_prep.hpp and chain_parse.hpp.
//
//   * layout          file f's bytes lie at file_off[f], a multiple of kTileBytes, and at least ONE byte follows every file:
//                     next_offset(off, len) = (off + len + 1) rounded up to a tile.  Every gap is filled with '\n' (pad_byte): that
//                     one byte closes an open comment and ends an unterminated last line, so a file boundary behaves like the end of
//                     a file and the comment-state scan needs no notion of files.
//   * lookups         file_of_tile / file_of_token: the last f with base[f] <= x (binary search; base has a sentinel entry, so an
//                     empty file -- base[f] == base[f + 1] -- is never the answer).
//   * byte classes    mce::chain_byte_class: what ends a line, separates fields, starts a comment (chain_kernels.hpp, the driver below).
//   * verdict         per file, inside its token range [t0, t1): ncols = tokens on the line of the first token; row r of the file
//                     is ragged if its ncols tokens do not share one line or the token before it lies on the same line;
//                     ntok % ncols != 0 is ragged too.  THE one statement of the rule: farm_files_kernel / farm_rows_kernel apply it
//                     per file of a wave, chain_ncols_kernel / chain_rows_kernel (the single-file reader) with t0 = 0.
//   * row table       a root is a list of parts (its files after burn-in); roots are numbered consecutively in one global row
//                     numbering: locate_row maps a global row to (root, part, local row).
// farm_structure is the serial driver: the same functions over a whole wave on one CPU thread.
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

#include <vector>

#include "seg_tiles.hpp"

namespace mce {

enum : int { kByteOther = 0, kByteSpace = 1, kByteTerm = 2, kByteHash = 3 };

MCE_HD inline __attribute__((always_inline)) int chain_byte_class(unsigned c)
{
    if (c == '\n' || c == '\r') return kByteTerm;
    if (c == ' ' || c == '\t' || c == '\v' || c == '\f') return kByteSpace;
    return c == '#' ? kByteHash : kByteOther;
}

}  // namespace mce

namespace mce_farm {

constexpr int64_t kTileBytes = 4096;      // = mce::kChainTileBytes (static_assert in chain_farm_kernels.hpp)
constexpr char kPadByte = '\n';

// where the file after one of `len` bytes at `off` starts
MCE_HD inline int64_t next_offset(int64_t off, int64_t len) { return (off + len + 1 + kTileBytes - 1) / kTileBytes * kTileBytes; }

// is (file_off, file_len)[nfiles] a layout of a wave of `wave_bytes` bytes?  (offsets on tiles, the first at 0, a pad byte behind every
// file, the wave a whole number of tiles)
inline bool layout_ok(const int64_t* file_off, const int64_t* file_len, int64_t nfiles, int64_t wave_bytes)
{
    if (nfiles < 1 || wave_bytes < kTileBytes || wave_bytes % kTileBytes != 0) return false;
    for (int64_t f = 0; f < nfiles; ++f) {
        if (file_len[f] < 0 || file_off[f] < 0 || file_off[f] % kTileBytes != 0) return false;
        if (f == 0 && file_off[0] != 0) return false;
        const int64_t next = f + 1 < nfiles ? file_off[f + 1] : wave_bytes;
        if (file_len[f] > wave_bytes || next < next_offset(file_off[f], file_len[f])) return false;
    }
    return true;
}

// the last f in [0, n) with base[f] <= x; base[0] <= x is the caller's promise (base is non-decreasing): seg_tiles.hpp's search
MCE_HD inline int64_t last_at_or_below(const int64_t* base, int64_t n, int64_t x)
{
    return mce_seg::last_at_or_below(n, x, [base](int64_t i) { return base[i]; });
}

// file_tile0[f] = file_off[f] / kTileBytes
MCE_HD inline int64_t file_of_tile(const int64_t* file_tile0, int64_t nfiles, int64_t tile) { return last_at_or_below(file_tile0, nfiles, tile); }
// tok0[f] = the file's first global token (non-decreasing; an empty file shares its value with the next file and is skipped)
MCE_HD inline int64_t file_of_token(const int64_t* tok0, int64_t nfiles, int64_t k) { return last_at_or_below(tok0, nfiles, k); }

// tokens on the line of token t0, inside [t0, t1) (tok_line is non-decreasing); 0 for an empty range
MCE_HD inline int64_t first_line_tokens(const int64_t* tok_line, int64_t t0, int64_t t1)
{
    if (t1 <= t0) return 0;
    const int64_t first = tok_line[t0];
    int64_t lo = t0, hi = t1;                     // first index whose line exceeds `first`
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (tok_line[mid] > first) hi = mid;
        else lo = mid + 1;
    }
    return lo - t0;
}

// row r (0 <= r < ntok / ncols) of the file whose tokens start at t0: do its ncols tokens fail to be exactly one line?
MCE_HD inline bool row_ragged(const int64_t* tok_line, int64_t t0, int64_t ncols, int64_t r)
{
    const int64_t k = t0 + r * ncols, line = tok_line[k];
    return tok_line[k + ncols - 1] != line || (r > 0 && tok_line[k - 1] == line);
}

struct FileVerdict {
    int64_t tok0 = 0, ntok = 0, nrows = 0, ncols = 0, ragged = 0;
};

// a file with no token has 0 rows and 0 columns
MCE_HD inline void file_counts(const int64_t* tok_line, int64_t t0, int64_t t1, FileVerdict* v)
{
    v->tok0 = t0;
    v->ntok = t1 - t0;
    v->ncols = first_line_tokens(tok_line, t0, t1);
    v->ragged = (v->ntok > 0 && v->ntok % v->ncols != 0) ? 1 : 0;
    v->nrows = v->ncols > 0 ? v->ntok / v->ncols : 0;
}

// ---- the row table of a wave's roots ------------------------------------------------------------------------------------------
// root r owns parts [part0[r], part0[r + 1]) and the global rows [row0[r], row0[r + 1]); part p holds the root-local rows
// [part_first[p], part_first[p] + part_rows[p]) (empty parts are allowed and never the answer).
struct RowPlace {
    int64_t root, part, local;      // local: the row inside the part
};

// the part of a root that holds the root-local row `in_root`: part_first[np] are the parts' first rows inside the root
MCE_HD inline int64_t part_of_row(const int64_t* part_first, int64_t np, int64_t in_root) { return last_at_or_below(part_first, np, in_root); }

MCE_HD inline RowPlace locate_row(const int64_t* row0, int64_t nroots, const int64_t* part0, const int64_t* part_first, int64_t g)
{
    RowPlace p;
    p.root = last_at_or_below(row0, nroots, g);
    const int64_t in_root = g - row0[p.root], pa = part0[p.root], np = part0[p.root + 1] - pa;
    p.part = pa + part_of_row(part_first + pa, np, in_root);
    p.local = in_root - part_first[p.part];
    return p;
}

// ---- serial driver -------------------------------------------------------------------------------------------------------------
// `text`: the wave as the device sees it (pads filled).  One serial scan gives the tokens' offsets and lines (the definition of
// chain_kernels.hpp: a token starts outside a comment at a byte that is neither space, line end nor '#' and follows a space, a line end
// or the start of the text); the per-file verdicts and the token -> file map come from the functions above.
inline void farm_structure(const unsigned char* text, int64_t wave_bytes, const int64_t* file_off, int64_t nfiles, std::vector<FileVerdict>* verdicts,
                           std::vector<int64_t>* tok_off, std::vector<int64_t>* tok_file)
{
    using namespace mce;
    std::vector<int64_t> tok_line, tile_tok((size_t)(wave_bytes / kTileBytes) + 1, 0);
    tok_off->clear();
    bool in_comment = false;
    int prev = kByteTerm;
    int64_t line = 0;
    for (int64_t i = 0; i < wave_bytes; ++i) {
        if (i % kTileBytes == 0) tile_tok[(size_t)(i / kTileBytes)] = (int64_t)tok_off->size();
        const int c = chain_byte_class(text[i]);
        if (c == kByteTerm) { in_comment = false; ++line; }
        else if (c == kByteHash) in_comment = true;
        else if (c == kByteOther && !in_comment && (prev == kByteSpace || prev == kByteTerm)) { tok_off->push_back(i); tok_line.push_back(line); }
        prev = c;
    }
    tile_tok[(size_t)(wave_bytes / kTileBytes)] = (int64_t)tok_off->size();
    verdicts->assign((size_t)nfiles, FileVerdict());
    std::vector<int64_t> tok0((size_t)nfiles);
    for (int64_t f = 0; f < nfiles; ++f) {
        const int64_t t0 = tile_tok[(size_t)(file_off[f] / kTileBytes)];
        const int64_t t1 = f + 1 < nfiles ? tile_tok[(size_t)(file_off[f + 1] / kTileBytes)] : (int64_t)tok_off->size();
        FileVerdict& v = (*verdicts)[(size_t)f];
        file_counts(tok_line.data(), t0, t1, &v);
        for (int64_t r = 0; r < v.nrows && !v.ragged; ++r)
            if (row_ragged(tok_line.data(), t0, v.ncols, r)) v.ragged = 1;
        tok0[(size_t)f] = t0;
    }
    tok_file->resize(tok_off->size());
    for (size_t k = 0; k < tok_off->size(); ++k) (*tok_file)[k] = file_of_token(tok0.data(), nfiles, (int64_t)k);
}

}  // namespace mce_farm
