// param_contours_check -- the serial drivers of mcevidence_amd/csrc/param_contours.hpp on the CPU
// (tests/test_param_contours_shared.py, tests/test_gpu_param_contours.py): the rule the device kernels follow.
//   param_contours_check contours <in> <out>   <in>: int64 np, double probs[np], int64 G, double scale, int64 nc, int64 cols[nc], then
//                                                    records {int64 n, int64 d, int64 ld, double x[n * ld], double w[n]};
//                                              <out>: per record the result block: con_out_doubles(nc, np, G) doubles
//   param_contours_check decide <in> <out>     <in>: int64 np, double probs[np], int64 G, then records {double lox, stepx, loy, stepy,
//                                                    double rho[G * G]}: a density array as some route formed it;
//                                              <out>: per record {mode_x, mode_y, mode_density, then per p: level, cells, lower_x,
//                                                    upper_x, lower_y, upper_y, edge}: steps 5 and 6 of the rule on that very array
//   param_contours_check parts                 the parts of a system's tiles and the order of the pairs
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "param_contours.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_parts()
{
    int count = 0;
    for (int64_t n : {0LL, 1LL, 511LL, 512LL, 513LL, 1025LL, 8192LL, 8193LL, 8705LL, 1000000LL, 2147483647LL}) {
        const int64_t nt = mce_seg::seg_ntiles(n);
        const int np = mce_con::con_nparts(n);
        if (np != (nt < 16 ? (int)nt : 16)) return 5;
        if (mce_con::con_part_tile(n, 0) != 0 || (np > 0 && mce_con::con_part_tile(n, np) != nt)) return 6;
        for (int p = 0; p < np; ++p)
            if (!(mce_con::con_part_tile(n, p) < mce_con::con_part_tile(n, p + 1))) return 7;
        ++count;
    }
    for (int nc = 2; nc <= mce_con::kConMaxCols; ++nc) {
        int p = 0;
        for (int s = 0; s < nc; ++s)
            for (int t = s + 1; t < nc; ++t, ++p)
                if (mce_con::con_pair_index(s, t, nc) != p) return 8;
        if (p != mce_con::con_npairs(nc)) return 8;
    }
    if (!mce_con::con_grid_ok(32) || !mce_con::con_grid_ok(64) || mce_con::con_grid_ok(16) || mce_con::con_grid_ok(128) || mce_con::con_grid_ok(48)) return 9;
    if (mce_con::con_out_doubles(27, 2, 64) != 8 + 9 * 27 + 351 * (4 + 14 + 4096)) return 10;
    printf("ok records=%d\n", count);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "parts")) return check_parts();
    const bool whole = argc >= 4 && !strcmp(argv[1], "contours"), decide = argc >= 4 && !strcmp(argv[1], "decide");
    if (whole || decide) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t np = 0, G = 0, count = 0;
        if (!get(in, &np) || np < 1 || np > mce_con::kConMaxP) return 3;
        std::vector<double> probs((size_t)np);
        if (!get(in, probs.data(), (size_t)np) || !get(in, &G) || !mce_con::con_grid_ok((int)G)) return 3;
        if (whole) {
            double scale = 0.0;
            int64_t nc = 0;
            if (!get(in, &scale) || !get(in, &nc) || !mce_con::con_nc_ok((int)nc)) return 3;
            std::vector<int64_t> cols64((size_t)nc);
            if (!get(in, cols64.data(), (size_t)nc)) return 3;
            std::vector<int32_t> cols(cols64.begin(), cols64.end());
            int64_t head[3];
            while (get(in, head, 3)) {
                const int64_t n = head[0], d = head[1], ld = head[2];
                if (n < 0 || n > (1 << 24) || d < 1 || d > mce_mar::kMarMaxDim || ld < d || ld > 4096) return 3;
                for (int64_t t = 0; t < nc; ++t)
                    if (cols[(size_t)t] < 0 || cols[(size_t)t] >= d || (t > 0 && cols[(size_t)t] <= cols[(size_t)t - 1])) return 3;
                std::vector<double> x((size_t)(n * ld)), w((size_t)n);
                if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size())) return 3;
                std::vector<double> res((size_t)mce_con::con_out_doubles((int)nc, (int)np, (int)G));
                mce_con::con_serial(x.data(), ld, n, (int)d, w.data(), cols.data(), (int)nc, probs.data(), (int)np, (int)G, scale, res.data());
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        } else {
            std::vector<double> rec((size_t)(G * G) + 4), res((size_t)(3 + mce_con::kConPerP * np));
            while (get(in, rec.data(), rec.size())) {
                mce_con::con_decide(rec.data() + 4, (int)G, rec[0], rec[1], rec[2], rec[3], probs.data(), (int)np, res.data(), res.data() + 3);
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: param_contours_check contours <in> <out> | decide <in> <out> | parts\n");
    return 1;
}
