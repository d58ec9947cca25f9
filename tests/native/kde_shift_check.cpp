// kde_shift_check -- the serial driver of mcevidence_amd/csrc/kde_shift.hpp on the CPU (tests/test_shift_kde_shared.py): the rule the
// device kernels follow, applied to whole systems, so that it can be compared with the oracle of tests/kde_cases.py.
//   kde_shift_check kde <in> <out>   <in>: records {int64 n, int64 d, int64 ld, double x[n * ld], double w[n], double linv[d * d],
//                                    double mean[d], double point[d], double c};
//                                    <out>: per record the result block (MCE_KDE_OUT doubles), the densities (n + 1) and the whitened
//                                    rows (n * d)
//   kde_shift_check parts            the parts of the reference range: for every n they tile the chunks without gaps, in order
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kde_shift.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_parts()
{
    using namespace mce_kde;
    int count = 0;
    for (int64_t n = 0; n <= 70000; n += (n < 2100 ? 1 : 997)) {
        const int np = kde_nparts(n);
        if (np < 1 || np > kKdeMaxParts) return 5;
        if (kde_part_chunk(n, 0) != 0 || kde_part_chunk(n, np) != kde_nchunks(n)) return 6;
        for (int p = 0; p < np; ++p)
            if (kde_part_chunk(n, p) > kde_part_chunk(n, p + 1) || (n > 0 && kde_part_chunk(n, p) == kde_part_chunk(n, p + 1))) return 7;
        ++count;
    }
    for (int d = 1; d <= kKdeMaxDim; ++d)
        if (kde_dpad(d) < d || kde_dpad(d) % 4 || kde_dpad(d) >= d + 4) return 8;
    printf("ok records=%d\n", count);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "parts")) return check_parts();
    if (argc >= 4 && !strcmp(argv[1], "kde")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t count = 0;
        int64_t head[3];
        while (get(in, head, 3)) {
            const int64_t n = head[0], d = head[1], ld = head[2];
            if (n < 0 || n > (1 << 20) || d < 1 || d > mce_kde::kKdeMaxDim || ld < d || ld > 4096) return 3;
            std::vector<double> x((size_t)(n * ld)), w((size_t)n), linv((size_t)(d * d)), mean((size_t)d), point((size_t)d);
            double c;
            if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size()) || !get(in, linv.data(), linv.size()) || !get(in, mean.data(), mean.size()) ||
                !get(in, point.data(), point.size()) || !get(in, &c))
                return 3;
            std::vector<double> res((size_t)mce_kde::kKdeOut), dens((size_t)n + 1), z((size_t)(n * d));
            mce_kde::kde_serial(x.data(), ld, n, (int)d, w.data(), linv.data(), mean.data(), point.data(), c, res.data(), dens.data(), z.data());
            fwrite(res.data(), sizeof(double), res.size(), out);
            fwrite(dens.data(), sizeof(double), dens.size(), out);
            if (!z.empty()) fwrite(z.data(), sizeof(double), z.size(), out);
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: kde_shift_check kde <in> <out> | parts\n");
    return 1;
}
