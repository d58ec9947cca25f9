// chain_parse_check.cpp -- the shared token parser (mcevidence_amd/csrc/chain_parse.hpp) on the CPU, as the device reader calls it:
//   chain_parse_check check FILE   every line of FILE is one token.  parse_token_exact (Clinger's fast path, then Eisel-Lemire) must
//                                  return the bits of strtod_l, or "undecided"; "rejected" only what strtod rejects as a whole token.
//                                  The host reader's parse_token must equal strtod_l always.  Prints
//                                  "ok n=<tokens> fast=<fast path alone> exact=<fast path + Eisel-Lemire> undecided=<left to strtod>".
//   chain_parse_check table        the 128-bit powers of five, one "q hi lo" line each (hex)
// Built by tests/test_chain_parse_shared.py with -fsanitize=undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "chain_parse.hpp"

using namespace mce_parse;

static uint64_t bits_of(double d)
{
    uint64_t b;
    std::memcpy(&b, &d, sizeof(b));
    return b;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "table")) {
        const uint64_t* t = pow5_table();
        for (int q = kPow5Min; q <= kPow5Max; ++q) std::printf("%d %016" PRIx64 " %016" PRIx64 "\n", q, t[2 * (q - kPow5Min)], t[2 * (q - kPow5Min) + 1]);
        return 0;
    }
    if (argc != 3 || std::strcmp(argv[1], "check")) {
        std::fprintf(stderr, "usage: chain_parse_check check FILE | table\n");
        return 2;
    }
    std::ifstream in(argv[2], std::ios::binary);
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    const uint64_t* pow5 = pow5_table();
    long long n = 0, fast = 0, exact = 0, undecided = 0, wrong = 0;
    std::string tok;
    while (std::getline(in, tok)) {
        ++n;
        const char* p = tok.data();
        const char* e = p + tok.size();
        double want = 0.0, got = 0.0, host = 0.0, f = 0.0;
        const bool want_ok = parse_slow(p, e, &want);
        const int rc = parse_token_exact(p, e, pow5, &got);
        const bool host_ok = parse_token(p, e, &host);
        bool bad = host_ok != want_ok || (host_ok && bits_of(host) != bits_of(want));
        if (rc == kConverted) {
            ++exact;
            bad |= !want_ok || bits_of(got) != bits_of(want);
        } else if (rc == kRejected) bad |= want_ok;
        else ++undecided;
        const int rf = parse_token_fast(p, e, &f);
        if (rf == kConverted) {
            ++fast;
            bad |= rc != kConverted || bits_of(f) != bits_of(got);
        }
        if (bad && ++wrong <= 20)
            std::printf("WRONG '%s': strtod %s %016" PRIx64 ", shared rc=%d %016" PRIx64 ", host reader %s %016" PRIx64 "\n", tok.c_str(), want_ok ? "ok" : "rejects",
                        bits_of(want), rc, bits_of(got), host_ok ? "ok" : "rejects", bits_of(host));
    }
    std::printf("%s n=%lld fast=%lld exact=%lld undecided=%lld wrong=%lld\n", wrong ? "FAIL" : "ok", n, fast, exact, undecided, wrong);
    return wrong ? 1 : 0;
}
