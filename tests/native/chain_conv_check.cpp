// chain_conv_check -- the serial driver of mcevidence_amd/csrc/chain_conv.hpp on the CPU (tests/test_chain_conv_shared.py): the rule
// the device kernels follow, applied to whole systems of segments, so that it can be compared with the oracle of tests/conv_cases.py.
//   chain_conv_check conv <in> <out>    <in>: records {int64 nseg, int64 ncols, int64 iw, int64 itheta, int64 ndim, then per segment:
//                                       int64 nrows, double rows[nrows * ncols]};
//                                       <out>: records {int64 status, column, used, skipped, double r_minus_1, double per_param[ndim]}
//                                       (per_param only where it was formed: status 0 or 4)
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chain_conv.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

template <class T>
static void put(FILE* f, const T* v, size_t count = 1)
{
    if (count) fwrite(v, sizeof(T), count, f);
}

int main(int argc, char** argv)
{
    if (argc >= 4 && !strcmp(argv[1], "conv")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t nseg, ncols, iw, itheta, ndim, count = 0;
        while (get(in, &nseg) && get(in, &ncols) && get(in, &iw) && get(in, &itheta) && get(in, &ndim)) {
            if (nseg < 1 || nseg > 1024 || ncols < 1 || ncols > 4096 || ndim < 1 || ndim > mce_conv::kConvMaxDim || itheta + ndim > ncols || iw < 0 ||
                iw >= ncols)
                return 3;
            std::vector<std::vector<double>> rows((size_t)nseg);
            std::vector<std::pair<const double*, int64_t>> segs;
            for (int64_t s = 0; s < nseg; ++s) {
                int64_t nr;
                if (!get(in, &nr) || nr < 0 || nr > (1 << 26)) return 3;
                rows[(size_t)s].resize((size_t)(nr * ncols));
                if (!get(in, rows[(size_t)s].data(), (size_t)(nr * ncols))) return 3;
                segs.emplace_back(rows[(size_t)s].data(), nr);
            }
            mce_conv::ConvResult r;
            mce_conv::conv_serial(segs, ncols, (int)iw, (int)itheta, (int)ndim, r);
            const int64_t head[4] = {r.status, r.column, r.used, r.skipped};
            put(out, head, 4);
            put(out, &r.r_minus_1);
            if (r.status == mce_conv::kConvOk || r.status == mce_conv::kConvNotPositive) put(out, r.per_param.data(), r.per_param.size());
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: chain_conv_check conv <in> <out>\n");
    return 1;
}
