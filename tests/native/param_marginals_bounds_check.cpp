// param_marginals_bounds_check -- the serial drivers of mcevidence_amd/csrc/param_marginals_bounds.hpp on the CPU
// (tests/test_param_marginals_bounds_shared.py, tests/test_gpu_param_marginals_bounds.py): the rule the device kernels follow.
//   param_marginals_bounds_check marginals <in> <out>   <in>: int64 np, double probs[np], int64 G, double scale, then records {int64 n,
//                                                      int64 d, int64 ld, double x[n * ld], double w[n], double lo[d], double hi[d]};
//                                                <out>: per record the result block: marb_out_doubles(d, np, G) doubles
//   param_marginals_bounds_check decide <in> <out>      <in>: int64 np, double probs[np], int64 G, then records {double lo, double step,
//                                                      double at_lo, double at_hi, double rho[G]}: a density array as some route formed it;
//                                                <out>: per record {mode, mode_density, then per p: lower, upper, pieces, edge}: steps 7'
//                                                      and 8' of the rule on that very array, serially
//   param_marginals_bounds_check consts                 the boundary constants of a column without bounds, and the layout
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "param_marginals_bounds.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_consts()
{
    using namespace mce_marb;
    int count = 0;
    const double inf = HUGE_VAL;
    for (double g : {-1e300, -3.5, 0.0, 0.015625, 7.0, 1e300})
        for (double h : {1e-300, 0.125, 1.0, 1e300}) {
            double a0, a1, a2, den;
            marb_consts(g, -inf, inf, h, &a0, &a1, &a2, &den);
            if (a0 != 1.0 || a1 != 0.0 || a2 != 1.0 || den != 1.0) return 5;
            for (double T0 : {0.0, 4.9e-324, 0.3, 1e300})
                for (double T1 : {-1e300, -0.25, 0.0, 2.0}) {
                    const double rho = marb_density(T0, T1, a0, a1, a2, den);
                    if (rho != T0 || std::signbit(rho)) return 6;
                }
            ++count;
        }
    if (marb_weighted(3.0, 0, 64, true, false) != 1.5 || marb_weighted(3.0, 63, 64, true, false) != 3.0 || marb_weighted(3.0, 63, 64, false, true) != 1.5 ||
        marb_weighted(3.0, 5, 64, true, true) != 3.0)
        return 7;
    if (marb_out_doubles(3, 2, 64) != mar_out_doubles(3, 2, 64) + 4 * 3) return 8;
    if (marb_bounds_ok(1.0, 1.0) || marb_bounds_ok(2.0, 1.0) || marb_bounds_ok(__builtin_nan(""), 1.0) || marb_bounds_ok(0.0, __builtin_nan("")) ||
        marb_bounds_ok(inf, inf) || !marb_bounds_ok(-inf, inf) || !marb_bounds_ok(0.0, inf))
        return 9;
    if (marb_phi(40.0) != 0.0 || marb_psi(40.0) != 0.0 || !(marb_phi(0.0) > 0.39894) || marb_psi(0.0) != 0.0) return 10;
    printf("ok records=%d\n", count);
    return 0;
}

int main(int argc, char** argv)
{
    using namespace mce_marb;
    if (argc >= 2 && !strcmp(argv[1], "consts")) return check_consts();
    const bool whole = argc >= 4 && !strcmp(argv[1], "marginals"), decide = argc >= 4 && !strcmp(argv[1], "decide");
    if (whole || decide) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t np = 0, G = 0, count = 0;
        if (!get(in, &np) || np < 1 || np > kMarMaxP) return 3;
        std::vector<double> probs((size_t)np);
        if (!get(in, probs.data(), (size_t)np) || !get(in, &G) || !mar_grid_ok((int)G)) return 3;
        if (whole) {
            double scale = 0.0;
            if (!get(in, &scale)) return 3;
            int64_t head[3];
            while (get(in, head, 3)) {
                const int64_t n = head[0], d = head[1], ld = head[2];
                if (n < 0 || n > (1 << 24) || d < 1 || d > kMarMaxDim || ld < d || ld > 4096) return 3;
                std::vector<double> x((size_t)(n * ld)), w((size_t)n), b((size_t)(2 * d));
                if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size()) || !get(in, b.data(), b.size())) return 3;
                for (int64_t j = 0; j < d; ++j)
                    if (!marb_bounds_ok(b[(size_t)j], b[(size_t)(d + j)])) return 3;
                std::vector<double> res((size_t)marb_out_doubles((int)d, (int)np, (int)G));
                marb_serial(x.data(), ld, n, (int)d, w.data(), b.data(), probs.data(), (int)np, (int)G, scale, res.data());
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        } else {
            std::vector<double> rec((size_t)G + 4), res((size_t)(2 + kMarPerP * np));
            while (get(in, rec.data(), rec.size())) {
                marb_decide(rec.data() + 4, (int)G, rec[0], rec[1], rec[2] != 0.0, rec[3] != 0.0, probs.data(), (int)np, res.data(), res.data() + 2);
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: param_marginals_bounds_check marginals <in> <out> | decide <in> <out> | consts\n");
    return 1;
}
