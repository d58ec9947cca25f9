// param_summary_check -- the serial driver of mcevidence_amd/csrc/param_summary.hpp on the CPU (tests/test_param_summary_shared.py):
// the rule the device kernels follow, applied to whole systems, so that it can be compared with the exact model of
// tests/summary_cases.py.
//   param_summary_check summary <in> <out>   <in>: int64 nq, double q[nq], then records {int64 n, int64 d, int64 ld, int64 has_fs,
//                                                  double x[n * ld], double w[n], double fs[n] (if has_fs)};
//                                            <out>: per record the result block: MCE_SUMMARY_HEAD + d * (5 + nq) doubles
//   param_summary_check keys                 the key of a double and its inverse on a ladder of values: order and round trip
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "param_summary.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_keys()
{
    const double inf = std::numeric_limits<double>::infinity(), den = std::numeric_limits<double>::denorm_min();
    const double ladder[] = {-inf, -1e300, -1.0 - 2.220446049250313e-16, -1.0, -2.2250738585072014e-308, -den, 0.0, den, 2.2250738585072014e-308, 1.0,
                             1.0 + 2.220446049250313e-16, 1e300, inf};
    const int n = (int)(sizeof(ladder) / sizeof(ladder[0]));
    for (int i = 0; i < n; ++i) {
        if (mce_sum::sum_unkey(mce_sum::sum_key(ladder[i])) != ladder[i]) return 5;
        if (i > 0 && !(mce_sum::sum_key(ladder[i - 1]) < mce_sum::sum_key(ladder[i]))) return 6;
        if (!(mce_sum::sum_key(ladder[i]) < mce_sum::kSumPadKey)) return 7;
    }
    if (mce_sum::sum_key(-0.0) != mce_sum::sum_key(0.0)) return 8;
    printf("ok records=%d\n", n);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "keys")) return check_keys();
    if (argc >= 4 && !strcmp(argv[1], "summary")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t nq = 0, count = 0;
        if (!get(in, &nq) || nq < 1 || nq > MCE_SUMMARY_MAX_Q) return 3;
        std::vector<double> q((size_t)nq);
        if (!get(in, q.data(), (size_t)nq)) return 3;
        int64_t head[4];
        while (get(in, head, 4)) {
            const int64_t n = head[0], d = head[1], ld = head[2], has_fs = head[3];
            if (n < 0 || n > (1 << 24) || d < 1 || d > mce_sum::kSumMaxDim || ld < d || ld > 4096) return 3;
            std::vector<double> x((size_t)(n * ld)), w((size_t)n), fs((size_t)(has_fs ? n : 0));
            if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size()) || !get(in, fs.data(), fs.size())) return 3;
            std::vector<double> res((size_t)mce_sum::sum_out_doubles((int)d, (int)nq));
            mce_sum::sum_serial(x.data(), ld, n, (int)d, w.data(), has_fs ? fs.data() : nullptr, q.data(), (int)nq, res.data());
            fwrite(res.data(), sizeof(double), res.size(), out);
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: param_summary_check summary <in> <out> | keys\n");
    return 1;
}
