// div_check.cpp -- stand-alone host program around csrc/knn_div.hpp (the rule the k-NN relative entropy's kernels share), built by
// tests/test_divergence_shared.py with g++ -fsanitize=address,undefined.
//
//   div_check                       unit checks of the whitening, the entry groups, the short test, the term and the masses; prints "ok ..."
//   div_check <case.bin> <out.txt>  runs div_serial on a case the test wrote and writes its sums for the test to compare
// case.bin: int64 nq, L, nP, nQ, G, K, d, has_qid; then distP [nq][L] f64, idxP [nq][L] i64, distQ, idxQ likewise, qid [nq] i64 (if
// has_qid), gq [nq] i32, grP [nP] i32, grQ [nQ] i32 (if G > 0), aq [nq] f64, aP [nP] f64, bQ [nQ] f64.  out.txt: nshort, the short rows,
// the (G + 1) * K * 2 sums (%.17g).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "knn_div.hpp"

using namespace mce_div;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static int unit_checks()
{
    // the whitening: a lower-triangular factor, products added in column order
    const double linv[9] = {2.0, 0.0, 0.0, -1.0, 0.5, 0.0, 3.0, 1.0, 0.25}, mean[3] = {1.0, 2.0, 3.0}, x[3] = {2.0, 4.0, 7.0};
    CHECK(div_whiten_coord(linv, x, mean, 0) == 2.0);
    CHECK(div_whiten_coord(linv + 3, x, mean, 1) == -1.0 + 1.0);
    CHECK(div_whiten_coord(linv + 6, x, mean, 2) == 3.0 + 2.0 + 1.0);
    CHECK(div_finite(1.0) && !div_finite(NAN) && !div_finite(INFINITY));
    CHECK(div_bad_weight(0.0) && div_bad_weight(-1.0) && div_bad_weight(NAN) && div_bad_weight(INFINITY) && !div_bad_weight(0.5));
    // the entry groups: with groups as jack.hpp's, without them every entry that exists counts under group 0
    const int32_t gr[4] = {0, 1, 1, 2};
    CHECK(div_entry_group(3, 4, gr, -1) == 2 && div_entry_group(3, 4, gr, 3) == kJackSkip && div_entry_group(-1, 4, gr, -1) == kJackSkip);
    CHECK(div_entry_group(3, 4, nullptr, -1) == 0 && div_entry_group(4, 4, nullptr, -1) == kJackSkip && div_entry_group(2, 4, nullptr, 2) == kJackSkip);
    // the short test looks at both lists: auto 0 1 1 2, cross 1 1 0 missing
    const int ga[4] = {0, 1, 1, 2}, gb[4] = {1, 1, 0, kJackSkip};
    auto A = [&](int j) { return ga[j]; };
    auto B = [&](int j) { return gb[j]; };
    CHECK(!div_is_short(A, B, 4, 1, 3, 1));          // own group 1: deleting 0 or 2 leaves at least one entry in either list
    CHECK(div_is_short(A, B, 4, 1, 3, 3));           // deleting group 0 leaves 2 cross entries
    CHECK(div_is_short(A, B, 4, 0, 3, 2));           // deleting group 1 leaves 1 cross entry
    CHECK(!div_is_short(A, B, 4, -1, 0, 3) && div_is_short(A, B, 4, -1, 0, 4));          // no groups: the lists themselves
    // the term and the value
    CHECK(div_coincident(-INFINITY, 0.0) && div_coincident(1.0, std::log(0.0)) && !div_coincident(-700.0, 3.0));
    CHECK(std::fabs(div_s(3, std::log(2.0), std::log(0.5), 4.0, 2.0, std::log(8.0)) - (3.0 * std::log(4.0) + std::log(2.0) - std::log(8.0))) < 1e-15);
    CHECK(std::fabs(div_value(6.0, 1.0, 4.0, std::exp(1.0)) - 3.0) < 1e-15);
    // the masses
    const double a[5] = {1.0, 2.0, 4.0, 8.0, 16.0};
    const int32_t g[5] = {0, 1, 0, 2, 1};
    double m[4];
    div_masses(a, g, 5, 3, m);
    CHECK(m[0] == 31.0 && m[1] == 5.0 && m[2] == 18.0 && m[3] == 8.0);
    div_masses(a, nullptr, 5, 0, m);
    CHECK(m[0] == 31.0);
    std::printf("ok knn_div.hpp: whitening, entry groups, short test, term, masses\n");
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
    const int64_t nq = h[0], L = h[1], nP = h[2], nQ = h[3], G = h[4], K = h[5], d = h[6], has_qid = h[7];
    CHECK(nq >= 1 && L >= 1 && nP >= 1 && nQ >= 1 && (G == 0 || (G >= 2 && G <= mce_jack::kJackMaxGroups)) && K >= 1 && K <= kDivMaxK && K <= L && d >= 1);
    std::vector<double> dP, dQ, aq, aP, bQ;
    std::vector<int64_t> iP, iQ, qid;
    std::vector<int32_t> gq, grP, grQ;
    CHECK(read_vec(f, dP, (size_t)(nq * L)) && read_vec(f, iP, (size_t)(nq * L)) && read_vec(f, dQ, (size_t)(nq * L)) && read_vec(f, iQ, (size_t)(nq * L)));
    if (has_qid) CHECK(read_vec(f, qid, (size_t)nq));
    if (G > 0) CHECK(read_vec(f, gq, (size_t)nq) && read_vec(f, grP, (size_t)nP) && read_vec(f, grQ, (size_t)nQ));
    CHECK(read_vec(f, aq, (size_t)nq) && read_vec(f, aP, (size_t)nP) && read_vec(f, bQ, (size_t)nQ));
    std::fclose(f);
    std::vector<double> sums((size_t)((G + 1) * K * 2));
    std::vector<int64_t> rows((size_t)nq);
    const int64_t ns = div_serial(dP.data(), iP.data(), dQ.data(), iQ.data(), nq, (int)L, has_qid ? qid.data() : nullptr, G > 0 ? gq.data() : nullptr,
                                  G > 0 ? grP.data() : nullptr, nP, G > 0 ? grQ.data() : nullptr, nQ, (int)G, (int)K, (int)d, aq.data(), aP.data(), bQ.data(),
                                  sums.data(), rows.data());
    FILE* o = std::fopen(argv[2], "w");
    CHECK(o != nullptr);
    std::fprintf(o, "%lld\n", (long long)ns);
    for (int64_t i = 0; i < ns; ++i) std::fprintf(o, "%lld\n", (long long)rows[(size_t)i]);
    for (double x : sums) std::fprintf(o, "%.17g\n", x);
    std::fclose(o);
    return 0;
}
