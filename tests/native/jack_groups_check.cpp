// jack_groups_check -- the serial drivers of mcevidence_amd/csrc/jack_groups.hpp on the CPU (tests/test_jackknife_resident_shared.py): the
// rule the device kernels follow, so that it can be compared with jackknife.group_ids and with the exact model of tests/moments_cases.py
// applied to every deleted set.
//   jack_groups_check groups <in> <out>      <in>: records {int64 n, N, G, by, has_rows, has_src, nparts, int64 rows[n]?, int64 src[N]?,
//                                            int64 part_first[nparts]}; <out>: records {int32 g[n]}
//   jack_groups_check leave_out <in> <out>   <in>: records {int64 n, G, has_fs, double w[n], double fs[n]?, int32 g[n]};
//                                            <out>: records {int64 ok, double block[(G + 1) * 8]}
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jack_groups.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static const int64_t kMaxRows = 1 << 26;

int main(int argc, char** argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: jack_groups_check groups|leave_out <in> <out>\n");
        return 1;
    }
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int64_t count = 0;
    if (!strcmp(argv[1], "groups")) {
        int64_t h[7];
        while (get(in, h, 7)) {
            const int64_t n = h[0], N = h[1], G = h[2], by = h[3], has_rows = h[4], has_src = h[5], nparts = h[6];
            if (n < 0 || n > kMaxRows || N < 0 || N > kMaxRows || nparts < 0 || nparts > 64) return 3;
            std::vector<int64_t> rows((size_t)(has_rows ? n : 0)), src((size_t)(has_src ? N : 0)), first((size_t)nparts);
            if (!get(in, rows.data(), rows.size()) || !get(in, src.data(), src.size()) || !get(in, first.data(), first.size())) return 3;
            std::vector<int32_t> g((size_t)n);
            mce_jg::jg_groups_serial(has_rows ? rows.data() : nullptr, has_src ? src.data() : nullptr, nparts ? first.data() : nullptr, nparts, n, N, G, (int)by,
                                     g.data());
            fwrite(g.data(), sizeof(int32_t), g.size(), out);
            ++count;
        }
    } else if (!strcmp(argv[1], "leave_out")) {
        int64_t h[3];
        while (get(in, h, 3)) {
            const int64_t n = h[0], G = h[1], has_fs = h[2];
            if (n < 0 || n > kMaxRows || G < 1 || G > 64) return 3;
            std::vector<double> w((size_t)n), fs((size_t)(has_fs ? n : 0));
            std::vector<int32_t> g((size_t)n);
            if (!get(in, w.data(), w.size()) || !get(in, fs.data(), fs.size()) || !get(in, g.data(), g.size())) return 3;
            std::vector<double> block((size_t)(G + 1) * mce_jg::kJgOut, 0.0);
            const int64_t ok = mce_jg::jg_leave_out_serial(w.data(), has_fs ? fs.data() : nullptr, g.data(), n, (int)G, block.data()) ? 1 : 0;
            fwrite(&ok, sizeof(int64_t), 1, out);
            fwrite(block.data(), sizeof(double), block.size(), out);
            ++count;
        }
    } else {
        return 1;
    }
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("ok records=%lld\n", (long long)count);
    return 0;
}
