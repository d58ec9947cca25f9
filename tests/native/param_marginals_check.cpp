// param_marginals_check -- the serial drivers of mcevidence_amd/csrc/param_marginals.hpp on the CPU
// (tests/test_param_marginals_shared.py, tests/test_gpu_param_marginals.py): the rule the device kernels follow.
//   param_marginals_check marginals <in> <out>   <in>: int64 np, double probs[np], int64 G, double scale, then records {int64 n, int64 d,
//                                                      int64 ld, double x[n * ld], double w[n]};
//                                                <out>: per record the result block: mar_out_doubles(d, np, G) doubles
//   param_marginals_check decide <in> <out>      <in>: int64 np, double probs[np], int64 G, then records {double lo, double step,
//                                                      double rho[G]}: a density array as some route formed it;
//                                                <out>: per record {mode, mode_density, then per p: lower, upper, pieces, edge}: steps 5
//                                                      and 6 of the rule on that very array, serially
//   param_marginals_check parts                  the parts of a system's tiles: every tile in exactly one part, in order, none empty
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "param_marginals.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_parts()
{
    int count = 0;
    for (int64_t n : {0LL, 1LL, 511LL, 512LL, 513LL, 1025LL, 4100LL, 32768LL, 32769LL, 33300LL, 65536LL, 1000000LL, 2147483647LL}) {
        const int64_t nt = mce_seg::seg_ntiles(n);
        const int np = mce_mar::mar_nparts(n);
        if (np != (nt < 64 ? (int)nt : 64)) return 5;
        if (mce_mar::mar_part_tile(n, 0) != 0 || (np > 0 && mce_mar::mar_part_tile(n, np) != nt)) return 6;
        for (int p = 0; p < np; ++p)
            if (!(mce_mar::mar_part_tile(n, p) < mce_mar::mar_part_tile(n, p + 1))) return 7;
        ++count;
    }
    for (int G : {64, 128, 256, 512, 1024})
        if (!mce_mar::mar_grid_ok(G) || mce_mar::mar_nblocks(G) != (G + 255) / 256) return 8;
    if (mce_mar::mar_grid_ok(0) || mce_mar::mar_grid_ok(100) || mce_mar::mar_grid_ok(2048)) return 9;
    if (mce_kde::kde_kernel_arg_value(746.0) != 0.0 || !(mce_kde::kde_kernel_arg_value(744.0) > 0.0)) return 10;
    printf("ok records=%d\n", count);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "parts")) return check_parts();
    const bool whole = argc >= 4 && !strcmp(argv[1], "marginals"), decide = argc >= 4 && !strcmp(argv[1], "decide");
    if (whole || decide) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t np = 0, G = 0, count = 0;
        if (!get(in, &np) || np < 1 || np > mce_mar::kMarMaxP) return 3;
        std::vector<double> probs((size_t)np);
        if (!get(in, probs.data(), (size_t)np) || !get(in, &G) || !mce_mar::mar_grid_ok((int)G)) return 3;
        if (whole) {
            double scale = 0.0;
            if (!get(in, &scale)) return 3;
            int64_t head[3];
            while (get(in, head, 3)) {
                const int64_t n = head[0], d = head[1], ld = head[2];
                if (n < 0 || n > (1 << 24) || d < 1 || d > mce_mar::kMarMaxDim || ld < d || ld > 4096) return 3;
                std::vector<double> x((size_t)(n * ld)), w((size_t)n);
                if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size())) return 3;
                std::vector<double> res((size_t)mce_mar::mar_out_doubles((int)d, (int)np, (int)G));
                mce_mar::mar_serial(x.data(), ld, n, (int)d, w.data(), probs.data(), (int)np, (int)G, scale, res.data());
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        } else {
            std::vector<double> rec((size_t)G + 2), res((size_t)(2 + mce_mar::kMarPerP * np));
            while (get(in, rec.data(), rec.size())) {
                mce_mar::mar_decide(rec.data() + 2, (int)G, rec[0], rec[1], probs.data(), (int)np, res.data(), res.data() + 2);
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: param_marginals_check marginals <in> <out> | decide <in> <out> | parts\n");
    return 1;
}
