// seg_tiles_check -- the segment-tile scheme of mcevidence_amd/csrc/seg_tiles.hpp on the CPU (tests/test_seg_tiles_shared.py): the
// table builder, the tile lookup and the keyed search that the statistics kernels share, over segment lists drawn from the row counts
// {0, 1, 511, 512, 513, 1024, 1025, 4100}.
//   seg_tiles_check all
// Prints "ok lists=<count> tiles=<count> keys=<count>" last; the first failed check prints its line and ends the run with status 1.
// Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "chain_farm.hpp"
#include "seg_tiles.hpp"

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

struct Seg {
    int64_t n;
};
struct Keyed {
    int64_t pad, key;
};

static long long g_tiles = 0, g_keys = 0;

// the last i with keys[i] <= x, by a scan from the front
static int64_t scan_last(const std::vector<int64_t>& keys, int64_t x)
{
    int64_t at = 0;
    for (size_t i = 0; i < keys.size(); ++i)
        if (keys[i] <= x) at = (int64_t)i;
    return at;
}

// every key from the first entry to two above the last: the keyed form over a struct member with both index types, and the array form
static void check_search(const std::vector<int64_t>& keys)
{
    std::vector<Keyed> table;
    for (int64_t k : keys) table.push_back(Keyed{-1, k});
    const Keyed* t = table.data();
    for (int64_t x = keys.front(); x <= keys.back() + 2; ++x) {
        const int64_t want = scan_last(keys, x);
        CHECK(mce_seg::last_at_or_below((int64_t)keys.size(), x, [t](int64_t i) { return t[i].key; }) == want);
        CHECK(mce_seg::last_at_or_below((int)keys.size(), x, [t](int i) { return t[i].key; }) == (int)want);
        CHECK(mce_farm::last_at_or_below(keys.data(), (int64_t)keys.size(), x) == want);
        ++g_keys;
    }
}

static void check_list(const std::vector<int64_t>& rows)
{
    mce_seg::SegTable T;
    std::vector<Seg> segs;
    for (int64_t n : rows) {
        T.add(n);
        segs.push_back(Seg{n});
    }
    // tile0 and ntiles by a direct count
    int64_t count = 0, nrows = 0;
    CHECK(T.tile0.size() == rows.size());
    for (size_t s = 0; s < rows.size(); ++s) {
        CHECK(T.tile0[s] == count);
        int64_t mine = 0;
        for (int64_t r = 0; r < rows[s]; r += 512) ++mine;
        CHECK(mce_seg::seg_ntiles(rows[s]) == mine);
        count += mine;
        nrows += rows[s];
    }
    CHECK(T.ntiles == count && T.nrows == nrows && T.fits());
    CHECK(count <= mce_seg::seg_max_tiles(nrows, (int64_t)rows.size()));
    // every tile maps to a segment with rows, and a segment's tiles are its rows 0 .. n, in order, once each
    std::vector<int64_t> next(rows.size(), 0), owned(rows.size(), 0);
    int64_t before = 0;
    for (int64_t tile = 0; tile < T.ntiles; ++tile) {
        int64_t r0 = -1, r1 = -1;
        const int64_t s = mce_seg::seg_tile_rows(segs.data(), T.tile0.data(), (int)rows.size(), tile, r0, r1);
        CHECK(s >= before && s < (int64_t)rows.size());
        before = s;
        CHECK(rows[(size_t)s] > 0);
        CHECK(r0 == next[(size_t)s] && r1 > r0 && r1 - r0 <= 512 && r1 <= rows[(size_t)s]);
        CHECK(r1 - r0 == 512 || r1 == rows[(size_t)s]);
        next[(size_t)s] = r1;
        owned[(size_t)s] += 1;
        ++g_tiles;
    }
    for (size_t s = 0; s < rows.size(); ++s) {
        CHECK(next[s] == rows[s]);
        CHECK(owned[s] == mce_seg::seg_ntiles(rows[s]));
        if (rows[s] == 0) CHECK(owned[s] == 0);
    }
    check_search(T.tile0);
}

int main(int argc, char** argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: seg_tiles_check all\n");
        return 1;
    }
    const int64_t C[8] = {0, 1, 511, 512, 513, 1024, 1025, 4100};
    long long lists = 0;
    // every list of one, two and three segments
    for (int a = 0; a < 8; ++a) {
        check_list({C[a]});
        ++lists;
        for (int b = 0; b < 8; ++b) {
            check_list({C[a], C[b]});
            ++lists;
            for (int c = 0; c < 8; ++c) {
                check_list({C[a], C[b], C[c]});
                ++lists;
            }
        }
    }
    // an empty segment first, in the middle and last; two side by side; empty segments only; all the counts, forwards and backwards
    const std::vector<std::vector<int64_t>> more = {
        {0, 513, 1024, 4100},       {513, 0, 1024, 1},           {1, 4100, 511, 0},     {512, 0, 0, 1025}, {0, 0, 4100, 0, 0, 1, 0, 0},
        {0},                        {0, 0, 0, 0, 0},             {0, 1, 511, 512, 513, 1024, 1025, 4100},  {4100, 1025, 1024, 513, 512, 511, 1, 0},
        {1, 1, 1, 1, 1, 1, 1, 1, 1}, {0, 1, 0, 1, 0, 1, 0, 511, 0}};
    for (const std::vector<int64_t>& rows : more) {
        check_list(rows);
        ++lists;
    }
    // runs of equal keys, and keys above the last entry, apart from any table
    check_search({0, 0, 0});
    check_search({0, 3, 3, 3, 7, 7, 20});
    check_search({5});
    check_search({0, 1, 2, 3, 4, 5, 6, 6});
    // 2^40 rows in one segment are 2^31 tiles: refused; 2^40 - 512 rows are 2^31 - 1: accepted.  No row is touched.
    {
        mce_seg::SegTable big, fit;
        big.add((int64_t)1 << 40);
        CHECK(big.ntiles == (int64_t)1 << 31 && !big.fits());
        fit.add(((int64_t)1 << 40) - 512);
        CHECK(fit.ntiles == 0x7fffffffLL && fit.fits());
        const Seg seg{((int64_t)1 << 40) - 512};
        int64_t r0, r1;
        CHECK(mce_seg::seg_tile_rows(&seg, fit.tile0.data(), 1, fit.ntiles - 1, r0, r1) == 0 && r0 == seg.n - 512 && r1 == seg.n);
        // the refusal counts the call's tiles, not a segment's
        mce_seg::SegTable two;
        two.add(((int64_t)1 << 40) - 512);
        two.add(1);
        CHECK(!two.fits());
    }
    printf("ok lists=%lld tiles=%lld keys=%lld\n", lists, g_tiles, g_keys);
    return 0;
}
