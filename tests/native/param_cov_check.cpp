// param_cov_check -- the serial driver of mcevidence_amd/csrc/param_cov.hpp on the CPU (tests/test_param_cov_shared.py): the rule the
// device kernels follow, applied to whole systems, so that it can be compared with the exact model of tests/cov_cases.py.
//   param_cov_check cov <in> <out>   <in>: records {int64 n, int64 d, int64 ld, double x[n * ld], double w[n]};
//                                    <out>: per record the result block: MCE_COV_HEAD + d + d (d + 1) / 2 doubles
//   param_cov_check blocks           the block order and the packed triangle: every (i, j), i <= j < d, is in exactly one block and has
//                                    its own slot, for every d
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "param_cov.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_blocks()
{
    using namespace mce_cov;
    for (int d = 1; d <= kCovMaxDim; ++d) {
        const int nb = cov_nblk(d), nblk = cov_nblocks(d);
        if (nblk > kCovMaxBlocks) return 5;
        std::vector<int> seen((size_t)cov_tri_doubles(d), 0);
        for (int p = 0; p < nblk; ++p) {
            int bi, bj;
            cov_block(p, nb, &bi, &bj);
            if (bi < 0 || bi > bj || bj >= nb) return 6;
            for (int t = 0; t < kCovBlock * kCovBlock; ++t) {
                const int i = kCovBlock * bi + t / kCovBlock, j = kCovBlock * bj + t % kCovBlock;
                if (i <= j && j < d) seen[(size_t)cov_tri(i, j, d)] += 1;
            }
        }
        for (int v : seen)
            if (v != 1) return 7;
        if (cov_tri(d - 1, d - 1, d) != cov_tri_doubles(d) - 1 || cov_tri(0, 0, d) != 0) return 8;
    }
    printf("ok records=%d\n", kCovMaxDim);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "blocks")) return check_blocks();
    if (argc >= 4 && !strcmp(argv[1], "cov")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t count = 0;
        int64_t head[3];
        while (get(in, head, 3)) {
            const int64_t n = head[0], d = head[1], ld = head[2];
            if (n < 0 || n > (1 << 24) || d < 1 || d > mce_cov::kCovMaxDim || ld < d || ld > 4096) return 3;
            std::vector<double> x((size_t)(n * ld)), w((size_t)n);
            if (!get(in, x.data(), x.size()) || !get(in, w.data(), w.size())) return 3;
            std::vector<double> res((size_t)mce_cov::cov_out_doubles((int)d));
            mce_cov::cov_serial(x.data(), ld, n, (int)d, w.data(), res.data());
            fwrite(res.data(), sizeof(double), res.size(), out);
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: param_cov_check cov <in> <out> | blocks\n");
    return 1;
}
