// chain_corr_check -- the serial driver of mcevidence_amd/csrc/chain_corr.hpp on the CPU (tests/test_chain_corr_shared.py): the rules
// the device kernels call, applied to whole chains, so that they can be compared with the oracle and with chains.correlation_length.
//   chain_corr_check corr <in> <out>    <in>: records {int64 nparts, int64 ncols, int64 iw, int64 itheta, int64 ndim, double min_corr,
//                                       int64 max_lag, then per part: int64 nrows, double rows[nrows * ncols]};
//                                       <out>: records {int64 rule, status, column, units, max_units, cap, rho_rows, double L,
//                                       double length[ndim], int64 cut[ndim], double rho[rho_rows * ndim]} (nothing after rule for a decline;
//                                       length / cut / rho only where they were formed: status 0 or 1)
//   chain_corr_check map <in> <out>     <in>: records {int64 n, double w[n]}; <out>: records {int64 units, int64 row[units]}: the row of
//                                       every unit by corr_unit_row, for w as ONE part and again as the second of two parts
//   chain_corr_check factor <scale> <length>      prints corr_factor
// Prints "ok records=<count>" last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "chain_corr.hpp"

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
    if (argc >= 4 && !strcmp(argv[1], "factor")) {
        printf("%lld\n", (long long)mce_corr::corr_factor(atof(argv[2]), atof(argv[3])));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "corr")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t nparts, ncols, iw, itheta, ndim, max_lag, count = 0;
        double min_corr;
        while (get(in, &nparts) && get(in, &ncols) && get(in, &iw) && get(in, &itheta) && get(in, &ndim) && get(in, &min_corr) && get(in, &max_lag)) {
            if (nparts < 1 || nparts > 1024 || ncols < 1 || ncols > 4096 || ndim < 1 || itheta + ndim > ncols || iw < 0 || iw >= ncols) return 3;
            std::vector<std::vector<double>> rows((size_t)nparts);
            std::vector<std::pair<const double*, int64_t>> parts;
            for (int64_t p = 0; p < nparts; ++p) {
                int64_t nr;
                if (!get(in, &nr) || nr < 0 || nr > (1 << 26)) return 3;
                rows[(size_t)p].resize((size_t)(nr * ncols));
                if (!get(in, rows[(size_t)p].data(), (size_t)(nr * ncols))) return 3;
                parts.emplace_back(rows[(size_t)p].data(), nr);
            }
            mce_corr::CorrResult r;
            mce_corr::corr_serial(parts, ncols, (int)iw, (int)itheta, (int32_t)ndim, min_corr, max_lag, r);
            const int64_t head[7] = {r.rule, r.status, r.column, r.units, r.max_units, r.cap, r.rho_rows};
            put(out, head, r.rule < 0 ? 1 : 7);
            if (r.rule >= 0) {
                put(out, &r.L);
                const bool formed = r.status == mce_corr::kCorrOk || r.status == mce_corr::kCorrNoCut;
                if (formed) {
                    put(out, r.length.data(), r.length.size());
                    put(out, r.cut.data(), r.cut.size());
                    put(out, r.rho.data(), r.rho.size());
                }
            }
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "map")) {
        FILE* in = fopen(argv[2], "rb");
        FILE* out = fopen(argv[3], "wb");
        if (!in || !out) return 2;
        int64_t n, count = 0;
        while (get(in, &n)) {
            if (n < 0 || n > (1 << 26)) return 3;
            std::vector<double> w((size_t)n);
            if (!get(in, w.data(), (size_t)n)) return 3;
            // the weights twice in one concatenated numbering: part 0 = rows [0, n), part 1 = rows [n, 2 n)
            std::vector<int64_t> c((size_t)(2 * n));
            int64_t run = 0;
            for (int64_t i = 0; i < 2 * n; ++i) c[(size_t)i] = (run += mce_prep::weight_int(w[(size_t)(i % n)]));
            const int64_t units = n > 0 ? c[(size_t)n - 1] : 0;
            put(out, &units);
            for (int part = 0; part < 2; ++part)
                for (int64_t u = 0; u < units; ++u) {
                    const int64_t row = mce_corr::corr_unit_row(c.data(), part * n, n, part ? units : 0, u);
                    put(out, &row);
                }
            ++count;
        }
        fclose(in);
        if (fclose(out) != 0) return 4;
        printf("ok records=%lld\n", (long long)count);
        return 0;
    }
    fprintf(stderr, "usage: chain_corr_check corr <in> <out> | map <in> <out> | factor <scale> <length>\n");
    return 1;
}
