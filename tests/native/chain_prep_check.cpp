// chain_prep_check -- the serial driver of mcevidence_amd/csrc/chain_prep.hpp on the CPU (tests/test_chain_prep_shared.py): the
// per-element rules the device kernels call, applied to whole weight vectors, so that they can be compared with chains.py.
//   chain_prep_check select <in> <out>    <in>: records {int64 n, double thinlen, int64 force (0: the header chooses the rule), int64 nedges,
//                                         double w[n], double edges[nedges]};
//                                         <out>: records {int64 rule, int64 nout, int64 keep[nout], double new_w[nout]}
//   chain_prep_check burn <in>            <in>: records {int64 nrows, double burn}; prints one start per line
// Prints "ok records=<count>" last.  Built with -fsanitize=undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_prep.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "burn")) {
        FILE* in = fopen(argv[2], "rb");
        if (!in) return 2;
        int64_t nrows, count = 0;
        double burn;
        while (get(in, &nrows) && get(in, &burn)) {
            printf("%lld\n", (long long)mce_prep::burn_start(nrows, burn));
            ++count;
        }
        fclose(in);
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "select")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t n, nedges, force, count = 0;
        double thinlen;
        std::vector<double> w, edges, new_w;
        std::vector<int64_t> keep;
        while (get(in, &n) && get(in, &thinlen) && get(in, &force) && get(in, &nedges)) {
            if (n < 0 || nedges < 0 || n > (1 << 28) || nedges > (1 << 28)) return 3;
            w.resize((size_t)n);
            edges.resize((size_t)nedges);
            if (!get(in, w.data(), (size_t)n) || !get(in, edges.data(), (size_t)nedges)) return 3;
            const int64_t rule = mce_prep::thin_select(w.data(), n, thinlen, edges.data(), nedges, keep, new_w, (int)force);
            const int64_t nout = (int64_t)keep.size();
            fwrite(&rule, sizeof(rule), 1, out);
            fwrite(&nout, sizeof(nout), 1, out);
            if (nout) {
                fwrite(keep.data(), sizeof(int64_t), (size_t)nout, out);
                fwrite(new_w.data(), sizeof(double), (size_t)nout, out);
            }
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: chain_prep_check select <in> <out> | burn <in>\n");
    return 1;
}
