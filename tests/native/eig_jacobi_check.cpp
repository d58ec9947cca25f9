// eig_jacobi_check -- the rules of mcevidence_amd/csrc/eig_jacobi.hpp on the CPU (tests/test_eig_shared.py): the pair schedule the
// device solver walks, and its serial driver (and, for comparison, the host solver) on whole matrices.
//   eig_jacobi_check schedule             for every d in 1..128: each unordered pair of real indices exactly once per sweep, the
//                                         pairs of one step disjoint, a bye only with the padding slot; prints "ok schedule"
//   eig_jacobi_check solve <in> <out>     <in>: records {int64 d, int64 solver (0: tournament driver, 1: jacobi_eig), double a[d*d]};
//                                         <out>: records {int64 status[4], double lam[d], double scale[d], double evec[d*d]}
//                                         (jacobi_eig: its eigenvalues and vectors, status by the shared rule, no counters)
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <vector>

#include "eig_jacobi.hpp"

template <class T>
static bool get(FILE* f, T* v, size_t count = 1)
{
    return count == 0 || fread(v, sizeof(T), count, f) == count;
}

static int check_schedule()
{
    for (int d = 1; d <= 128; ++d) {
        const int m = mce_eig::slots(d), np = mce_eig::pairs_per_step(d), ns = mce_eig::steps_per_sweep(d);
        if (m != d + (d & 1) || np != m / 2 || ns != m - 1) return 1;
        std::vector<int> seen((size_t)d * d, 0);
        for (int step = 0; step < ns; ++step) {
            std::vector<int> used((size_t)m, 0);
            for (int k = 0; k < np; ++k) {
                int p = -1, q = -1;
                mce_eig::pair_of(d, step, k, p, q);
                if (p < 0 || q <= p || q >= m) return 2;
                if (used[p]++ || used[q]++) return 3;            // not disjoint
                if (q >= d) {
                    if (!(d & 1) || q != d) return 4;            // a bye without a padding slot
                    continue;
                }
                ++seen[(size_t)p * d + q];
            }
            for (int i = 0; i < m; ++i)
                if (used[i] != 1) return 5;                      // every slot plays in every step
        }
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q)
                if (seen[(size_t)p * d + q] != 1) return 6;
    }
    printf("ok schedule\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "schedule")) return check_schedule();
    if (argc >= 4 && !strcmp(argv[1], "solve")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t d, solver, count = 0;
        while (get(in, &d) && get(in, &solver)) {
            if (d < 1 || d > 1024) return 3;
            const size_t dd = (size_t)d * d;
            std::vector<double> a(dd), evec(dd), scale((size_t)d), lam((size_t)d);
            if (!get(in, a.data(), dd)) return 3;
            int32_t st[mce_eig::kStatInts] = {0, 0, 0, 0};
            if (solver == 0) {
                mce_eig::tournament_eig(a.data(), (int)d, evec.data(), scale.data(), lam.data(), st);
            } else {
                std::vector<double> A(a), l, V;
                mce_eig::jacobi_eig(A, (int)d, l, V);
                int index = 0;
                st[mce_eig::kStatCode] = mce_eig::status_of(l.data(), (int)d, index);
                st[mce_eig::kStatIndex] = index;
                for (int64_t i = 0; i < d; ++i) {
                    lam[i] = l[i];
                    scale[i] = 1.0 / std::sqrt(l[i]);
                }
                evec = V;
            }
            const int64_t st64[4] = {st[0], st[1], st[2], st[3]};
            fwrite(st64, sizeof(int64_t), 4, out);
            fwrite(lam.data(), sizeof(double), (size_t)d, out);
            fwrite(scale.data(), sizeof(double), (size_t)d, out);
            fwrite(evec.data(), sizeof(double), dd, out);
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: eig_jacobi_check schedule | solve <in> <out>\n");
    return 2;
}
