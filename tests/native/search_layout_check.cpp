// search_layout_check.cpp -- csrc/search_layout.hpp on the CPU: the arenas of one nearest-neighbour search (PruneArena, SymArena, SearchArena in
// its four shapes, PairsOnceArena) hold on a grid of sizes, and at the pins they are, byte for byte, what the planner counted by hand.
//   search_layout_check <pins file>
// The grid: every family; d in 1, 2, 15, 16, 63, 64, 127, 128, 1024; nq, nr in 1, 31, 32, 513, 70 000; K in 1, 4, 16, 17, 32, 33; the pruned
// walk, its heavy waves' side lists and the symmetric sweep off and on; S in 1, 3 chains of the pairs-once share.  Asserted: every array
// starts on a multiple of 256 bytes; the arrays follow each other in the documented order without overlap, each with room for the content its
// line documents; the sizing pass (no base) equals the placing pass; bucket_cnt | bucket_flag | done are contiguous; cf32 lies inside Xs
// exactly when Xs is large enough.  The pins (tests/golden/search_layout_pins.txt) are the lines a throw-away program printed from the
// library at 3aad787, the last commit whose make_plan / prune_layout / sym_layout / pairs_once_shape counted offsets by hand: the plan's
// numbers, every offset and total, and the rocPRIM temporary-storage sizes it saw -- which go in here as inputs, so no pin depends on rocPRIM.
#include "search_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace mce;

namespace {

char* const kBase = reinterpret_cast<char*>((uintptr_t)1 << 44);      // never dereferenced
long g_grid = 0, g_pins = 0;

#define REQUIRE(c, ...)                                                         \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #c);             \
            fprintf(stderr, __VA_ARGS__);                                       \
            fprintf(stderr, "\n");                                              \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

struct Item { const char* name; const void* p; size_t bytes; };

// the items lie in order from `base`, 256-aligned, each with room for `bytes`, inside `total`
void check_row(const char* what, const std::vector<Item>& items, const char* base, size_t total)
{
    const char* end = base;
    for (const Item& it : items) {
        const char* p = static_cast<const char*>(it.p);
        REQUIRE(p != nullptr, "%s.%s is null", what, it.name);
        REQUIRE((size_t)(p - base) % 256 == 0, "%s.%s at %zu", what, it.name, (size_t)(p - base));
        REQUIRE(p >= end, "%s.%s at %zu overlaps the array before it (ends %zu)", what, it.name, (size_t)(p - base), (size_t)(end - base));
        REQUIRE((size_t)(p - end) < 256 || end == base, "%s.%s: a gap of %zu bytes", what, it.name, (size_t)(p - end));
        end = p + it.bytes;
    }
    REQUIRE((size_t)(end - base) <= total && total - (size_t)(end - base) < 256, "%s: total %zu, content ends %zu", what, total, (size_t)(end - base));
    REQUIRE(total % 256 == 0, "%s: total %zu", what, total);
}

void check_prune(const SearchSizes& z, const PruneArena& A, const char* base)
{
    const size_t nmax = (size_t)std::max(z.nq_pad, z.nrow_pad), nbig = (size_t)std::max(z.nq, z.nr), d = (size_t)z.d;
    const size_t tr = (size_t)z.nrow_pad / 32, tq = (size_t)z.nq_pad / 32, nw = (size_t)z.nqblk * 8, pairs = (size_t)z.nqblk * (size_t)z.nchunk;
    const bool in_xs = (size_t)z.nq * d * 8 >= nbig * d * 4;
    std::vector<Item> it = {{"perm_r", A.perm_r, (size_t)z.nrow_pad * 4}, {"perm_q", A.perm_q, (size_t)z.nq_pad * 4}, {"keys_a", A.keys_a, nmax * 8},
                            {"keys_b", A.keys_b, nmax * 8}, {"vals_b", A.vals_b, nmax * 4}, {"Ys", A.Ys, (size_t)z.nr * d * 8}, {"Xs", A.Xs, (size_t)z.nq * d * 8}};
    if (!in_xs) it.push_back({"cf32", A.cf32, nbig * d * 4});
    const std::vector<Item> rest = {{"tbox_r", A.tbox_r, tr * 2 * d * 4}, {"tbox_q", A.tbox_q, tq * 2 * d * 4}, {"tboxT_r", A.tboxT_r, tr * 2 * d * 4},
                                    {"box_r", A.box_r, (size_t)z.nchunk * 2 * d * 4}, {"box_q", A.box_q, (size_t)z.nqblk * 2 * d * 4}, {"bkey_a", A.bkey_a, nw * 4},
                                    {"bkey_b", A.bkey_b, nw * 4}, {"bval_a", A.bval_a, nw * 4}, {"border", A.border, nw * 4}, {"list_d", A.list_d, pairs * 4},
                                    {"list_c", A.list_c, pairs * 4}, {"tmp", A.tmp, z.prune_tmp_bytes}};
    it.insert(it.end(), rest.begin(), rest.end());
    check_row("prune", it, base, A.total);
    REQUIRE(A.cf32_in_Xs == in_xs, "cf32 rule");
    if (in_xs) REQUIRE((void*)A.cf32 == (void*)A.Xs && nbig * d * 4 <= (size_t)z.nq * d * 8, "cf32 inside Xs");
    else REQUIRE((char*)A.cf32 >= (char*)A.Xs + (size_t)z.nq * d * 8, "cf32 behind Xs");
    REQUIRE(PruneArena(z).total == A.total, "prune: sizing pass %zu, placing pass %zu", PruneArena(z).total, A.total);
}

void check_sym(const SearchSizes& z, const SymArena& A, const char* base)
{
    const size_t n = (size_t)z.nq_pad;
    check_row("sym", {{"perm", A.perm, n * 4}, {"keys_a", A.keys_a, n * 4}, {"keys_b", A.keys_b, n * 4}, {"vals_a", A.vals_a, n * 4},
                      {"Ys", A.Ys, (size_t)z.nr * z.d * 8}, {"thr", A.thr, n * 8}, {"rrow", A.rrow, n * 4}, {"rtile", A.rtile, n / 32 * 4},
                      {"slots", A.slots, n * z.KCAP * 8}, {"counters", A.counters, (size_t)z.nqblk * 12},
                      {"bucket", A.bucket, (size_t)z.nqblk * z.sym_cap * 16}, {"tmp", A.tmp, z.sym_tmp_bytes}}, base, A.total);
    REQUIRE(A.bucket_cnt() == A.counters && A.bucket_flag() == A.counters + z.nqblk && A.done() == A.counters + 2 * z.nqblk &&
            A.counters_bytes() == (size_t)z.nqblk * 12 && A.cap == z.sym_cap, "the three counters are one array");
    REQUIRE(SymArena(z).total == A.total, "sym: sizing pass %zu, placing pass %zu", SymArena(z).total, A.total);
}

void check_search(const SearchSizes& z, const SearchArena& A, char* base)
{
    const size_t lists = (size_t)z.list_sets * z.KCAP * (size_t)z.nq_pad;
    const Item pd{"pd", A.pd, lists * 8}, pi{"pi", A.pi, lists * 4}, center{"center", A.center, z.center_doubles * 8}, msum{"msum", A.msum, z.msum_doubles * 8};
    const Item yf{"yf", A.yf, (size_t)z.nrow_pad * z.KS * 32}, yfl{"yfl", A.yfl, (size_t)z.nrow_pad * z.KS * 32};
    std::vector<Item> it;
    switch (z.family) {
    case SearchFamily::long_rows:
        it = {pd, pi, center, msum, yfl, {"xf", A.xf, (size_t)z.nq_pad * z.KS * 32}, {"xn", A.xn, (size_t)z.nq_pad * 8}, {"slack", A.slack, 256}};
        break;
    case SearchFamily::generic:
        it = {pd, pi, {"dist", A.dist, (size_t)z.nq * z.K * 8}, {"slack", A.slack, 256}};
        break;
    case SearchFamily::sweep64:
        it = {yf, pd, pi, center, msum};
        break;
    case SearchFamily::filter:
        it = {{"yh", A.yh, (size_t)z.nrow_pad * 16 * z.KST * 2}, {"xh", A.xh, (size_t)z.nq_pad * 16 * z.KST * 2}, {"qinfo", A.qinfo, (size_t)z.nq_pad * 16},
              {"params", A.params, z.params_doubles * 8}, pd, pi, center, msum};
        if (z.prune) {
            it.push_back({"prune", A.prune.perm_r, A.prune.total});
            check_prune(z, A.prune, (const char*)A.prune.perm_r);
            if (z.heavy_max > 0) {
                it.push_back({"heavy", A.heavy_d, A.heavy_entries * 12});
                REQUIRE((char*)A.heavy_i() == (char*)A.heavy_d + A.heavy_entries * 8 && A.heavy_entries == (size_t)z.heavy_max * z.heavy_cols * z.KCAP, "heavy: distances | rows");
            }
        }
        if (z.sym) {
            it.push_back({"sym", A.sym.perm, A.sym.total});
            check_sym(z, A.sym, (const char*)A.sym.perm);
        }
        break;
    }
    check_row("search", it, base, A.total);
    REQUIRE((z.prune && z.heavy_max > 0) == (A.heavy_d != nullptr) && A.lists().d == A.pd && A.lists().i == A.pi, "heavy / lists");
    const SearchArena Z(z);
    REQUIRE(Z.total == A.total && Z.pd == nullptr && Z.prune.perm_r == nullptr && Z.sym.thr == nullptr && Z.heavy_i() == nullptr && Z.sym.done() == nullptr && (A.yf == nullptr || A.yfl == nullptr),
            "search: sizing pass %zu, placing pass %zu", Z.total, A.total);
}

void check_pairs_once(const SearchSizes& z, size_t dotp_bytes, int S)
{
    const PairsOnceArena W(z, dotp_bytes, S, kBase), Z(z, dotp_bytes, S);
    check_search(z, W.A, kBase);
    std::vector<Item> it = {{"search", W.search, W.A.total}, {"partial", W.partial, dotp_bytes}};
    if (S > 1) { it.push_back({"sets_d", W.sets_d, W.set_entries() * 8}); it.push_back({"sets_i", W.sets_i, W.set_entries() * 4}); }
    check_row("pairs-once", it, kBase, W.total);
    REQUIRE(Z.total == W.total && W.search == kBase && (void*)W.A.yh == (void*)kBase, "pairs-once: sizing pass %zu, placing pass %zu", Z.total, W.total);
    REQUIRE(S > 1 ? (W.lists().d == W.sets_d && W.lists().i == W.sets_i) : (W.lists().d == W.A.pd && W.lists().i == W.A.pi && !W.sets_d && !W.sets_i), "lists()");
}

int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

void grid()
{
    const int ds[] = {1, 2, 15, 16, 63, 64, 127, 128, 1024}, Ks[] = {1, 4, 16, 17, 32, 33};
    const int64_t ns[] = {1, 31, 32, 513, 70000};
    for (int fam = 0; fam < 4; ++fam) for (int d : ds) for (int64_t nq : ns) for (int64_t nr : ns) for (int K : Ks)
        for (int opt = 0; opt < (fam == 3 ? 4 : 1); ++opt) {          // filter: plain, pruned walk, ... with heavy waves, symmetric sweep
            SearchSizes z;
            z.family = (SearchFamily)fam;
            z.nq = nq; z.nr = nr; z.d = d; z.K = K;
            const int qpb = fam == 0 ? 256 : fam == 1 ? 128 : 512, chunk = opt == 1 || opt == 2 ? 2048 : 1536;
            z.nqblk = (int)((nq + qpb - 1) / qpb); z.nq_pad = (int64_t)z.nqblk * qpb;
            z.nrow_pad = round_up(nr, chunk); z.nchunk = z.nrow_pad / chunk;
            z.KS = (d + 3) / 4; z.KST = (d + 15) / 16; z.KCAP = fam == 1 ? K : K <= 4 ? 4 : K <= 8 ? 8 : K <= 12 ? 12 : K <= 16 ? 16 : 32;
            z.list_sets = fam == 1 ? 1 : 1 + (int)((nq + K) % 5);
            z.center_doubles = fam == 0 ? (size_t)d + 4 : fam == 1 ? 0 : 192; z.msum_doubles = fam == 0 ? (size_t)256 * d : fam == 1 ? 0 : 49152;
            z.params_doubles = fam == 3 ? 16 : 0;
            if (opt == 1 || opt == 2) { z.prune = true; z.prune_tmp_bytes = (size_t)(nq * 7 + nr * 3 + 1); }
            if (opt == 2) { z.heavy_max = 32 + z.nqblk / 2; z.heavy_cols = 448; }
            if (opt == 3) { z.sym = true; z.sym_cap = 78 * qpb; z.sym_tmp_bytes = (size_t)(nq * 5 + 3); }
            check_search(z, SearchArena(z, kBase), kBase);
            ++g_grid;
            if (opt == 3)
                for (int S : {1, 3}) { check_pairs_once(z, (size_t)round_up(((nr + 255) / 256) * (K + 1) * 8, 256), S); ++g_grid; }
        }
}

// ---- the pins ----
typedef std::map<std::string, long long> Rec;
Rec parse(const std::string& text)
{
    Rec r;
    size_t i = 0;
    while (i < text.size()) {
        size_t j = text.find(' ', i);
        if (j == std::string::npos) j = text.size();
        const std::string tok = text.substr(i, j - i);
        const size_t eq = tok.find('=');
        if (eq != std::string::npos) r[tok.substr(0, eq)] = atoll(tok.c_str() + eq + 1);
        i = j + 1;
    }
    return r;
}
long long at(const Rec& r, const char* key)
{
    const auto it = r.find(key);
    REQUIRE(it != r.end(), "pin without %s", key);
    return it->second;
}
#define PIN(ptr, key) REQUIRE((char*)(ptr) - base == at(r, key), "%s: %s at %lld, pinned %lld", name.c_str(), key, (long long)((char*)(ptr) - base), at(r, key))

void pin(const std::string& line)
{
    const size_t c0 = line.find(" :: "), c1 = line.find(" | PL "), c2 = line.find(" | SL "), c3 = line.find(" | APO ");
    REQUIRE(line.compare(0, 4, "PIN ") == 0 && c0 != std::string::npos, "not a pin: %s", line.c_str());
    const std::string name = line.substr(4, line.find(' ', 4) - 4);
    const size_t e0 = std::min(std::min(c1, c2), std::min(c3, line.size()));
    const Rec r = parse(line.substr(c0 + 4, e0 - c0 - 4));
    Rec pl, sl, apo;
    if (c1 != std::string::npos) pl = parse(line.substr(c1 + 6, std::min(c2, std::min(c3, line.size())) - c1 - 6));
    if (c2 != std::string::npos) sl = parse(line.substr(c2 + 6, std::min(c3, line.size()) - c2 - 6));
    if (c3 != std::string::npos) apo = parse(line.substr(c3 + 7));
    const int fam = (int)at(r, "fam");
    SearchSizes z;
    z.family = (SearchFamily)fam;
    z.nq = at(r, "nq"); z.nr = at(r, "nr"); z.d = (int)at(r, "d"); z.K = (int)at(r, "K");
    z.nq_pad = at(r, "nq_pad"); z.nrow_pad = at(r, "nrow_pad"); z.nchunk = at(r, "nchunk"); z.nqblk = (int)at(r, "nqblk");
    z.KS = (int)at(r, "KS"); z.KST = (int)at(r, "KST"); z.KCAP = (int)at(r, "KCAP");
    z.list_sets = fam == 1 ? 1 : (int)std::max(at(r, "L"), at(r, "sym_nsplit"));
    z.center_doubles = fam == 0 ? (size_t)z.d + 4 : fam == 1 ? 0 : 192; z.msum_doubles = fam == 0 ? (size_t)256 * z.d : fam == 1 ? 0 : 49152;
    z.params_doubles = fam == 3 ? 16 : 0;
    z.prune = at(r, "prune") != 0; z.sym = at(r, "sym") != 0;
    REQUIRE(z.prune == !pl.empty() && z.sym == !sl.empty(), "%s: sub-arena records", name.c_str());
    if (z.prune) z.prune_tmp_bytes = (size_t)at(pl, "tmp_bytes");
    z.heavy_max = (int)at(r, "heavy_max"); z.heavy_cols = z.heavy_max ? 448 : 0;
    if (z.sym) { z.sym_tmp_bytes = (size_t)at(sl, "tmp_bytes"); z.sym_cap = (int)at(sl, "cap"); }
    char* const base = kBase;
    const SearchArena A(z, base);
    check_search(z, A, base);
    REQUIRE((long long)A.total == at(r, "total"), "%s: total %zu, pinned %lld", name.c_str(), A.total, at(r, "total"));
    PIN(A.pd, "pd"); PIN(A.pi, "pi");
    if (fam == 0) { PIN(A.center, "center"); PIN(A.msum, "msum"); PIN(A.yfl, "yf"); PIN(A.xf, "xf"); PIN(A.xn, "xn"); }
    if (fam == 1) PIN(A.dist, "center");          // (the hand-counted generic plan kept its distance scratch in off_center)
    if (fam == 2) { PIN(A.yf, "yf"); PIN(A.center, "center"); PIN(A.msum, "msum"); }
    if (fam == 3) { PIN(A.yh, "yh"); PIN(A.xh, "xh"); PIN(A.qinfo, "qinfo"); PIN(A.params, "params"); PIN(A.center, "center"); PIN(A.msum, "msum"); }
    if (z.prune) {
        PIN(A.prune.perm_r, "prune_off");
        if (z.heavy_max) PIN(A.heavy_d, "heavy_off");
        const Rec& r = pl;
        char* const base = (char*)A.prune.perm_r;
        const PruneArena& P = A.prune;
        PIN(P.perm_r, "perm_r"); PIN(P.perm_q, "perm_q"); PIN(P.keys_a, "keys_a"); PIN(P.keys_b, "keys_b"); PIN(P.vals_b, "vals_b"); PIN(P.Ys, "Ys"); PIN(P.Xs, "Xs");
        PIN(P.cf32, "cf32"); PIN(P.tbox_r, "tbox_r"); PIN(P.tbox_q, "tbox_q"); PIN(P.tboxT_r, "tboxT_r"); PIN(P.box_r, "box_r"); PIN(P.box_q, "box_q");
        PIN(P.bkey_a, "bkey_a"); PIN(P.bkey_b, "bkey_b"); PIN(P.bval_a, "bval_a"); PIN(P.border, "border"); PIN(P.list_d, "list_d"); PIN(P.list_c, "list_c");
        PIN(P.tmp, "tmp");
        REQUIRE((long long)P.total == at(r, "total"), "%s: prune total", name.c_str());
    }
    if (z.sym) {
        PIN(A.sym.perm, "sym_off");
        const Rec& r = sl;
        char* const base = (char*)A.sym.perm;
        const SymArena& S = A.sym;
        PIN(S.perm, "perm"); PIN(S.keys_a, "keys_a"); PIN(S.keys_b, "keys_b"); PIN(S.vals_a, "vals_a"); PIN(S.Ys, "Ys"); PIN(S.thr, "thr"); PIN(S.rrow, "rrow");
        PIN(S.rtile, "rtile"); PIN(S.slots, "slots"); PIN(S.bucket_cnt(), "cnt"); PIN(S.bucket_flag(), "flag"); PIN(S.done(), "done"); PIN(S.bucket, "bucket");
        PIN(S.tmp, "tmp");
        REQUIRE((long long)S.total == at(r, "total"), "%s: sym total", name.c_str());
    }
    if (!apo.empty()) {
        const Rec& r = apo;
        const int S = (int)at(r, "nsplit");
        check_pairs_once(z, (size_t)at(r, "dotp"), S);
        const PairsOnceArena W(z, (size_t)at(r, "dotp"), S, base);
        PIN(W.lists().d, "off_d"); PIN(W.lists().i, "off_i");
        REQUIRE((long long)W.total == at(r, "total") && (char*)W.partial - base == (long long)A.total, "%s: pairs-once total", name.c_str());
    }
    ++g_pins;
}

}  // namespace

int main(int argc, char** argv)
{
    REQUIRE(argc == 2, "usage: %s <pins file>", argv[0]);
    grid();
    FILE* f = fopen(argv[1], "r");
    REQUIRE(f != nullptr, "cannot read %s", argv[1]);
    std::vector<char> buf(1 << 16);
    while (fgets(buf.data(), (int)buf.size(), f)) {
        std::string line(buf.data());
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (!line.empty() && line[0] != '#') pin(line);
    }
    fclose(f);
    printf("ok grid=%ld pins=%ld\n", g_grid, g_pins);
    return 0;
}
