// like_moments_check -- the serial driver of mcevidence_amd/csrc/like_moments.hpp on the CPU (tests/test_like_moments_shared.py): the
// rule the device kernels follow, applied to whole systems, so that it can be compared with the exact model of tests/moments_cases.py.
//   like_moments_check moments <in> <out>    <in>: records {int64 n, double fs[n], double w[n]};
//                                            <out>: records {double W, c, v, A2, rows used, status}
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "like_moments.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

int main(int argc, char** argv)
{
    if (argc >= 4 && !strcmp(argv[1], "moments")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t n, count = 0;
        while (get(in, &n)) {
            if (n < 0 || n > (1 << 26)) return 3;
            std::vector<double> fs((size_t)n), w((size_t)n);
            if (!get(in, fs.data(), (size_t)n) || !get(in, w.data(), (size_t)n)) return 3;
            double res[mce_mom::kMomOut];
            mce_mom::mom_serial(fs.data(), w.data(), n, res);
            fwrite(res, sizeof(double), mce_mom::kMomOut, out);
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: like_moments_check moments <in> <out>\n");
    return 1;
}
