// chain_farm_check -- the serial driver of mcevidence_amd/csrc/chain_farm.hpp on the CPU (tests/test_chain_farm_shared.py): the layout,
// the per-file verdicts, the token -> file map and the row-table lookups the device kernels call.
//   chain_farm_check structure <in> <out>   <in>: records {int64 nfiles, int64 len[nfiles], bytes of every file one after the other};
//                                           the wave is laid out with next_offset, gaps filled with the pad byte, garbage ('7') never
//                                           left in a gap; <out>: per record {int64 wave_bytes, int64 off[nfiles], per file {int64 nrows,
//                                           ncols, ragged, tok0, ntok}, int64 ntok, int64 tok_file[ntok], int64 tok_off_in_file[ntok]}
//   chain_farm_check alone <in> <out>       <in>: as for structure; <out>: per record and file {int64 nrows, ncols, ragged, ntok} inside the
//                                           wave, then the same four for the file as a wave of its own (nfiles = 1, its tokens from
//                                           t0 = 0: the calls the single-file reader's kernels make)
//   chain_farm_check rows <in> <out>        <in>: records {int64 nroots, int64 nparts[nroots], int64 part_rows[sum nparts]};
//                                           <out>: per record {int64 nrows, then per global row {int64 root, part, local}}
// Prints "ok records=<count>" last.  Built with -fsanitize=undefined,address.
#include <cstdio>
#include <cstring>
#include <vector>

#include "chain_farm.hpp"

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
    if (argc < 4) return 2;
    FILE* in = fopen(argv[2], "rb");
    FILE* out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    int64_t count = 0;
    const bool alone = !strcmp(argv[1], "alone");
    if (alone || !strcmp(argv[1], "structure")) {
        int64_t nfiles;
        while (get(in, &nfiles)) {
            if (nfiles < 1 || nfiles > (1 << 20)) return 3;
            std::vector<int64_t> len((size_t)nfiles), off((size_t)nfiles);
            if (!get(in, len.data(), (size_t)nfiles)) return 3;
            int64_t at = 0;
            for (int64_t f = 0; f < nfiles; ++f) {
                if (len[(size_t)f] < 0 || len[(size_t)f] > (1 << 28)) return 3;
                off[(size_t)f] = at;
                at = mce_farm::next_offset(at, len[(size_t)f]);
            }
            const int64_t wave = at;
            std::vector<unsigned char> text((size_t)wave, (unsigned char)mce_farm::kPadByte);
            for (int64_t f = 0; f < nfiles; ++f)
                if (!get(in, text.data() + off[(size_t)f], (size_t)len[(size_t)f])) return 3;
            if (!mce_farm::layout_ok(off.data(), len.data(), nfiles, wave)) return 5;
            std::vector<mce_farm::FileVerdict> v;
            std::vector<int64_t> tok_off, tok_file;
            mce_farm::farm_structure(text.data(), wave, off.data(), nfiles, &v, &tok_off, &tok_file);
            if (alone) {
                for (int64_t f = 0; f < nfiles; ++f) {
                    const int64_t zero = 0, w1 = mce_farm::next_offset(0, len[(size_t)f]);
                    std::vector<unsigned char> one((size_t)w1, (unsigned char)mce_farm::kPadByte);
                    memcpy(one.data(), text.data() + off[(size_t)f], (size_t)len[(size_t)f]);
                    std::vector<mce_farm::FileVerdict> v1;
                    mce_farm::farm_structure(one.data(), w1, &zero, 1, &v1, &tok_off, &tok_file);
                    if (v1[0].tok0 != 0) return 6;
                    const int64_t rec[8] = {v[(size_t)f].nrows, v[(size_t)f].ncols, v[(size_t)f].ragged, v[(size_t)f].ntok,
                                            v1[0].nrows, v1[0].ncols, v1[0].ragged, v1[0].ntok};
                    put(out, rec, 8);
                }
                ++count;
                continue;
            }
            put(out, &wave);
            put(out, off.data(), (size_t)nfiles);
            for (int64_t f = 0; f < nfiles; ++f) {
                const int64_t rec[5] = {v[(size_t)f].nrows, v[(size_t)f].ncols, v[(size_t)f].ragged, v[(size_t)f].tok0, v[(size_t)f].ntok};
                put(out, rec, 5);
            }
            const int64_t ntok = (int64_t)tok_off.size();
            put(out, &ntok);
            put(out, tok_file.data(), (size_t)ntok);
            for (int64_t k = 0; k < ntok; ++k) tok_off[(size_t)k] -= off[(size_t)tok_file[(size_t)k]];
            put(out, tok_off.data(), (size_t)ntok);
            ++count;
        }
    } else if (!strcmp(argv[1], "rows")) {
        int64_t nroots;
        while (get(in, &nroots)) {
            if (nroots < 1 || nroots > (1 << 20)) return 3;
            std::vector<int64_t> np((size_t)nroots), row0((size_t)nroots + 1, 0), part0((size_t)nroots + 1, 0);
            if (!get(in, np.data(), (size_t)nroots)) return 3;
            for (int64_t r = 0; r < nroots; ++r) part0[(size_t)r + 1] = part0[(size_t)r] + np[(size_t)r];
            const int64_t nparts = part0[(size_t)nroots];
            std::vector<int64_t> rows((size_t)nparts), first((size_t)nparts);
            if (!get(in, rows.data(), (size_t)nparts)) return 3;
            for (int64_t r = 0; r < nroots; ++r) {
                int64_t n = 0;
                for (int64_t p = part0[(size_t)r]; p < part0[(size_t)r + 1]; ++p) {
                    first[(size_t)p] = n;
                    n += rows[(size_t)p];
                }
                row0[(size_t)r + 1] = row0[(size_t)r] + n;
            }
            const int64_t n = row0[(size_t)nroots];
            put(out, &n);
            for (int64_t g = 0; g < n; ++g) {
                const mce_farm::RowPlace p = mce_farm::locate_row(row0.data(), nroots, part0.data(), first.data(), g);
                const int64_t rec[3] = {p.root, p.part, p.local};
                put(out, rec, 3);
            }
            ++count;
        }
    } else
        return 2;
    fclose(in);
    if (fclose(out) != 0) return 4;
    printf("ok records=%lld\n", (long long)count);
    return 0;
}
