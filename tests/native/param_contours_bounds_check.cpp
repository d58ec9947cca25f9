// param_contours_bounds_check -- the serial drivers of mcevidence_amd/csrc/param_contours.hpp with hard prior bounds on the CPU
// (tests/test_param_contours_bounds_shared.py, tests/test_gpu_param_contours_bounds.py): the rule the <true> kernels follow.
//   param_contours_bounds_check contours <in> <out>  <in>: int64 np, double probs[np], int64 G, double scale, int64 nc, int64 cols[nc], then
//                                                    records {int64 n, int64 d, int64 ld, double x[n * ld], double w[n], double lo[nc],
//                                                    double hi[nc]}; <out>: per record the result block: conb_out_doubles(nc, np, G) doubles
//   param_contours_bounds_check decide <in> <out>    <in>: int64 np, double probs[np], int64 G, then records {double lox, stepx, loy, stepy,
//                                                    x_at_lo, x_at_hi, y_at_lo, y_at_hi, double rho[G * G]}: a density array as some route
//                                                    formed it; <out>: per record {mode_x, mode_y, mode_density, then per p: level, cells,
//                                                    lower_x, upper_x, lower_y, upper_y, edge}: steps 7" and 8" on that very array
//   param_contours_bounds_check rule                 the pieces: an open pair's constants leave T00 as it is, the weights, the statuses
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

static int check_rule()
{
    using namespace mce_con;
    int count = 0;
    // a column that is open on both sides: a0 = 1, a1 = 0, a2 = 1, den = 1 at any grid point and h
    double u[4], v[4];
    for (double g : {-3.5, 0.0, 1e300}) {
        mce_marb::marb_consts(g, -HUGE_VAL, HUGE_VAL, 0.25, u, u + 1, u + 2, u + 3);
        if (!(u[0] == 1.0 && u[1] == 0.0 && u[2] == 1.0 && u[3] == 1.0)) return 5;
        ++count;
    }
    mce_marb::marb_consts(0.5, -HUGE_VAL, HUGE_VAL, 2.0, v, v + 1, v + 2, v + 3);
    // ... and the density of an open pair is T00, bit for bit, whatever it is
    for (double T00 : {0.1, 1.0 / 3.0, 5e-324, 1e-310, 1.7e308}) {
        if (conb_density(T00, 0.0, 0.0, u, v) != T00) return 6;
        ++count;
    }
    if (conb_density(0.0, 0.0, 0.0, u, v) != 0.0 || conb_density(-1.0, 0.0, 0.0, u, v) != 0.0) return 6;
    // one axis open: param_marginals_bounds.hpp's step 6' on the other, within a few roundings
    double a[4];
    mce_marb::marb_consts(0.25, 0.0, HUGE_VAL, 0.5, a, a + 1, a + 2, a + 3);
    const double T0 = 0.7, T1 = -0.2, want = mce_marb::marb_density(T0, T1, a[0], a[1], a[2], a[3]);
    const double gx = conb_density(T0, T1, 0.0, a, u), gy = conb_density(T0, 0.0, T1, u, a);
    if (!(fabs(gx - want) <= 1e-14 * want && fabs(gy - want) <= 1e-14 * want)) return 7;
    // a transposed pair of first moments is another number
    if (conb_density(T0, T1, 0.0, a, u) == conb_density(T0, 0.0, T1, a, u)) return 7;
    ++count;
    // the weights: 1, 1/2 or 1/4
    const int G = 32;
    if (conb_weighted(3.0, 0, G, true, false, true, false) != 0.75 || conb_weighted(3.0, 0, G, true, false, false, false) != 1.5 ||
        conb_weighted(3.0, G - 1, G, false, false, false, true) != 1.5 || conb_weighted(3.0, G * G - 1, G, false, true, false, true) != 0.75 ||
        conb_weighted(3.0, G + 1, G, true, true, true, true) != 3.0 || conb_weighted(3.0, 0, G, false, true, false, true) != 3.0)
        return 8;
    ++count;
    if (conb_pair_status(0, 0) != 0 || conb_pair_status(7, 8) != 7 || conb_pair_status(8, 7) != 8 || conb_pair_status(0, 8) != 8) return 9;
    if (conb_out_doubles(27, 2, 64) != 8 + 13 * 27 + 351 * (4 + 14 + 4096)) return 10;
    if (!conb_open(-HUGE_VAL, HUGE_VAL) || conb_open(0.0, HUGE_VAL) || conb_open(-HUGE_VAL, 0.0)) return 11;
    // step 3": 7 before 8; a grid that ends on the bound
    double sd, h, c, lo, step, at_lo, at_hi;
    if (conb_params(10.0, 10.0, 0.0, 1.0, 1.0, 2.0, 3.0, 1.0, 32, &sd, &h, &c, &lo, &step, &at_lo, &at_hi) != kConColBad) return 12;
    if (conb_params(10.0, 10.0, 1.0, 0.0, 4.0, 1.0, 5.0, 1.0, 32, &sd, &h, &c, &lo, &step, &at_lo, &at_hi) != kConbColOutside) return 12;
    if (conb_params(10.0, 10.0, 1.0, 0.0, 4.0, 0.0, HUGE_VAL, 1.0, 32, &sd, &h, &c, &lo, &step, &at_lo, &at_hi) != kConOk || lo != 0.0 || at_lo != 1.0 || at_hi != 0.0)
        return 12;
    ++count;
    printf("ok records=%d\n", count);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "rule")) return check_rule();
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
                std::vector<double> x((size_t)(n * ld)), w((size_t)n), bounds((size_t)(2 * nc));
                if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size()) || !get(in, bounds.data(), bounds.size())) return 3;
                for (int64_t t = 0; t < nc; ++t)
                    if (!mce_marb::marb_bounds_ok(bounds[(size_t)t], bounds[(size_t)(nc + t)])) return 3;
                std::vector<double> res((size_t)mce_con::conb_out_doubles((int)nc, (int)np, (int)G));
                mce_con::conb_serial(x.data(), ld, n, (int)d, w.data(), cols.data(), (int)nc, bounds.data(), probs.data(), (int)np, (int)G, scale, res.data());
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        } else {
            std::vector<double> rec((size_t)(G * G) + 8), res((size_t)(3 + mce_con::kConPerP * np));
            while (get(in, rec.data(), rec.size())) {
                const bool ends[4] = {rec[4] != 0.0, rec[5] != 0.0, rec[6] != 0.0, rec[7] != 0.0};
                mce_con::con_decide_ends(rec.data() + 8, (int)G, rec[0], rec[1], rec[2], rec[3], ends, probs.data(), (int)np, res.data(), res.data() + 3);
                fwrite(res.data(), sizeof(double), res.size(), out);
                ++count;
            }
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: param_contours_bounds_check contours <in> <out> | decide <in> <out> | rule\n");
    return 1;
}
