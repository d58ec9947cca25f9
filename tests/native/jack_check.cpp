// jack_check.cpp -- stand-alone host program around csrc/jack.hpp (the rule the jackknife kernels share), built by
// tests/test_jackknife_shared.py with g++ -fsanitize=address,undefined.
//
//   jack_check                       unit checks of the walk, the block rule and the two formulas; prints "ok ..."
//   jack_check <case.bin> <out.txt>  runs jack_serial on a case the test wrote and writes its sums for the test to compare
// case.bin: int64 nq, L, nr, G, k0, kmax, D, has_qid; then dist [nq][L] f64, idx [nq][L] i64, qid [nq] i64 (if has_qid), gq [nq] i32,
// gr [nr] i32, w [nq] f64, fs [nq] f64.  out.txt: nshort, the short rows, the G * kmax group sums, the kmax full sums (%.17g).
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "jack.hpp"

using namespace mce_jack;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int unit_checks()
{
    // the block rule: G contiguous stretches, sizes differing by at most one, every group in range
    for (int64_t N : {2, 7, 257, 300, 600, 1000003}) {
        for (int64_t G : {2, 8, 16, 64}) {
            std::vector<int64_t> cnt((size_t)G, 0);
            int prev = 0;
            for (int64_t r = 0; r < N; ++r) {
                const int g = jack_block_group(r, G, N);
                CHECK(g >= prev && g < G);
                prev = g;
                ++cnt[(size_t)g];
            }
            int64_t lo = N, hi = 0;
            for (int64_t c : cnt) { lo = c < lo ? c : lo; hi = c > hi ? c : hi; }
            CHECK(hi - lo <= 1);
        }
    }
    // the walk on one list: groups 0 1 1 self 2 1 0 missing
    const int32_t gr[6] = {0, 1, 1, 2, 1, 0};
    const int64_t idx[8] = {0, 1, 2, 9, 3, 4, 5, -1};
    auto group_at = [&](int j) { return jack_entry_group(idx[j] == 9 ? 9 : idx[j], idx[j] == 9 ? 10 : 6, gr, 9); };
    CHECK(group_at(3) == kJackSkip && group_at(7) == kJackSkip && group_at(4) == 2);
    {
        JackCursor c;                      // nothing deleted: 0 1 2 4 5 6
        const int want[6] = {0, 1, 2, 4, 5, 6};
        for (int k = 0; k < 6; ++k) CHECK(jack_next(group_at, 8, -1, c) == want[k]);
        CHECK(jack_next(group_at, 8, -1, c) == -1);
    }
    {
        JackCursor c;                      // group 1 deleted: 0 4 6
        const int want[3] = {0, 4, 6};
        for (int k = 0; k < 3; ++k) CHECK(jack_next(group_at, 8, 1, c) == want[k]);
        CHECK(jack_next(group_at, 8, 1, c) == -1);
    }
    CHECK(!jack_runs_out(group_at, 8, 1, 3) && jack_runs_out(group_at, 8, 1, 4));
    CHECK(!jack_is_short(group_at, 8, 1, 3, 4));          // own group 1 is not looked at: groups 0 and 2 leave 4 and 5
    CHECK(jack_is_short(group_at, 8, 0, 3, 4));           // group 1 deleted leaves 3
    CHECK(jack_is_short(group_at, 8, 1, 3, 7));           // the list itself holds 6
    // the formulas
    const double v[4] = {1.0, 2.0, 4.0, 5.0};
    CHECK(std::fabs(jack_mean(v, 4) - 3.0) < 1e-15);
    CHECK(std::fabs(jack_sigma(v, 4) - std::sqrt(0.75 * 10.0)) < 1e-15);
    CHECK(std::fabs(jack_bias_corrected(v, 4, 3.5) - (14.0 - 9.0)) < 1e-15);
    CHECK(std::fabs(jack_ln_unit_ball(2) - std::log(M_PI)) < 1e-15);
    std::printf("ok jack.hpp: block rule, walk, formulas\n");
    return 0;
}

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc < 3) return unit_checks();
    FILE* f = std::fopen(argv[1], "rb");
    CHECK(f != nullptr);
    int64_t h[8];
    CHECK(std::fread(h, sizeof(int64_t), 8, f) == 8);
    const int64_t nq = h[0], L = h[1], nr = h[2], G = h[3], k0 = h[4], kmax = h[5], D = h[6], has_qid = h[7];
    CHECK(nq >= 1 && L >= 1 && nr >= 1 && G >= 2 && G <= kJackMaxGroups && (k0 == 0 || k0 == 1) && kmax > k0 && kmax - k0 <= L && D >= 1);
    std::vector<double> dist, w, fs;
    std::vector<int64_t> idx, qid;
    std::vector<int32_t> gq, gr;
    CHECK(read_vec(f, dist, (size_t)(nq * L)) && read_vec(f, idx, (size_t)(nq * L)));
    if (has_qid) CHECK(read_vec(f, qid, (size_t)nq));
    CHECK(read_vec(f, gq, (size_t)nq) && read_vec(f, gr, (size_t)nr) && read_vec(f, w, (size_t)nq) && read_vec(f, fs, (size_t)nq));
    std::fclose(f);
    std::vector<double> groups((size_t)(G * kmax)), full((size_t)kmax);
    std::vector<int64_t> rows((size_t)nq);
    const int64_t ns = jack_serial(dist.data(), idx.data(), nq, (int)L, has_qid ? qid.data() : nullptr, gq.data(), gr.data(), nr, (int)G, (int)k0, (int)kmax,
                                   (int)D, w.data(), fs.data(), groups.data(), full.data(), rows.data());
    FILE* o = std::fopen(argv[2], "w");
    CHECK(o != nullptr);
    std::fprintf(o, "%lld\n", (long long)ns);
    for (int64_t i = 0; i < ns; ++i) std::fprintf(o, "%lld\n", (long long)rows[(size_t)i]);
    for (double x : groups) std::fprintf(o, "%.17g\n", x);
    for (double x : full) std::fprintf(o, "%.17g\n", x);
    std::fclose(o);
    return 0;
}
