// capi_farm.hpp -- part of capi.hip (one translation unit): mce_chain_farm_*: MANY chain files parsed in one pass per wave, and the
// preparation of the roots of a wave that are not thinned (chain_farm_kernels.hpp has the segmented passes, chain_farm.hpp the rules,
// chain_kernels.hpp the tile passes that run once over the whole wave).
//
// A farm reader handle is created once per device and serves every wave: ONE stream, device scratch sized for a capacity given at
// creation (the text, 26 bytes per 4 KB tile, 16 bytes per token of offsets and lines, the list of undecided tokens, the power table,
// 56 bytes per file) and ONE pinned staging buffer of the same capacity, which the caller fills.  No hipMalloc, hipFree or stream
// creation per file or per wave: an array a wave does not fit is grown once (counted in the stats).  A handle belongs to one thread.
// Per wave: one asynchronous upload, the pads, six structure launches, two per-file launches, one download of the per-file results
// (mce_chain_farm_structure: two synchronisations); one parse launch, the list's count and entries, one patch copy and launch
// (mce_chain_farm_parse: two synchronisations, three with patches).
#pragma once

#include "chain_farm.hpp"
#include "chain_farm_kernels.hpp"

namespace {

struct FarmDev : ReaderDev {
    int64_t capacity = 0, tile_cap = 0;
    char* staging = nullptr;                      // pinned, `capacity` bytes
    mce::ChainPatch* list = nullptr;          // the undecided tokens of a wave and their fixes
    double* fix = nullptr;
    size_t tok_cap = 0, list_cap = 0;
    // per file: offsets | lengths | first tiles (file_cap + 1 each), first tokens (file_cap + 1), verdicts (file_cap)
    int64_t* d_ftab = nullptr;
    int64_t* d_ftok0 = nullptr;
    mce_farm::FileVerdict* d_files = nullptr;
    size_t file_cap = 0;
    char* h_small = nullptr;                      // pinned: the file tables going up, the totals and verdicts coming down
    size_t h_small_cap = 0;
    // the wave in flight
    int64_t wave_bytes = 0, ntiles = 0, ntok = 0, nfiles = 0;
    std::vector<mce_farm::FileVerdict> verdicts;
    // statistics
    int64_t allocs = 0, allocs_wave = 0, grows = 0, waves = 0, files_total = 0, patched = 0;
    double ms_upload = 0.0, ms_structure = 0.0, ms_parse = 0.0, ms_patch = 0.0;

    ~FarmDev()          // (what the wave adds; ~ReaderDev frees the rest and the stream)
    {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != device) (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : {(void*)list, (void*)fix, (void*)d_ftab, (void*)d_ftok0, (void*)d_files})
            if (p) (void)hipFree(p);
        if (staging) (void)hipHostFree(staging);
        if (h_small) (void)hipHostFree(h_small);
        if (cur != device) (void)hipSetDevice(cur);
    }
};

// (re)allocate p for `count` elements; the stream is idle when an array grows (the callers synchronise before)
template <class T>
int farm_alloc(FarmDev& c, T*& p, size_t count, const char* what)
{
    if (p) {
        MCE_HIP(hipStreamSynchronize(c.stream));
        (void)hipFree(p);
        p = nullptr;
        ++c.grows;
    }
    ++c.allocs;
    ++c.allocs_wave;
    return chain_alloc(p, count, what);
}

int farm_reserve_files(FarmDev& c, size_t nfiles)
{
    if (nfiles <= c.file_cap && c.d_ftab) return MCE_OK;
    const size_t cap = std::max<size_t>(nfiles + nfiles / 2, 256);
    int rc;
    if ((rc = farm_alloc(c, c.d_ftab, 3 * (cap + 1), "the file table")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.d_ftok0, cap + 1, "the files' first tokens")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.d_files, cap, "the per-file results")) != MCE_OK) return rc;
    const size_t hb = 3 * (cap + 1) * sizeof(int64_t) + sizeof(mce::ChainTotals) + cap * sizeof(mce_farm::FileVerdict);
    if (c.h_small) (void)hipHostFree(c.h_small);
    c.h_small = nullptr;
    MCE_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.h_small), hb, hipHostMallocDefault));
    c.h_small_cap = hb;
    c.file_cap = cap;
    return MCE_OK;
}

// two arrays of one capacity, grown together to n + 25 % + 1024 elements when n do not fit
template <class A, class B>
int farm_reserve(FarmDev& c, size_t n, size_t& cap, A*& a, const char* what_a, B*& b, const char* what_b)
{
    if (n <= cap && a) return MCE_OK;
    const size_t grown = n + n / 4 + 1024;
    int rc;
    if ((rc = farm_alloc(c, a, grown, what_a)) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, b, grown, what_b)) != MCE_OK) return rc;
    cap = grown;
    return MCE_OK;
}

int farm_reserve_tokens(FarmDev& c, size_t ntok) { return farm_reserve(c, ntok, c.tok_cap, c.tok_off, "the token offsets", c.tok_line, "the token lines"); }
int farm_reserve_list(FarmDev& c, size_t n) { return farm_reserve(c, n, c.list_cap, c.list, "the list of undecided tokens", c.fix, "the patched values"); }

int farm_create(FarmDev& c)
{
    MCE_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    c.tile_cap = c.capacity / mce::kChainTileBytes;
    const size_t nt = (size_t)c.tile_cap;
    int rc;
    if ((rc = farm_alloc(c, c.text, (size_t)c.capacity, "the text")) != MCE_OK) return rc;
    MCE_HIP(hipHostMalloc(reinterpret_cast<void**>(&c.staging), (size_t)c.capacity, hipHostMallocDefault));
    if ((rc = farm_alloc(c, c.tile_kind, nt, "the tile states")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.tile_in, nt, "the tile states")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.tile_ntok, nt, "the tile counts")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.tile_nterm, nt, "the tile counts")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.tok_base, nt, "the tile offsets")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.term_base, nt, "the tile offsets")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.tot, 1, "the totals")) != MCE_OK) return rc;
    if ((rc = farm_alloc(c, c.pow5, (size_t)mce_parse::kPow5Words, "the powers of five")) != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(c.pow5, mce_parse::pow5_table(), (size_t)mce_parse::kPow5Words * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
    // chain text is seldom denser than one field per 8 bytes; one undecided token in 32 (capi_chain.hpp)
    if ((rc = farm_reserve_tokens(c, (size_t)c.capacity / 8)) != MCE_OK) return rc;
    if ((rc = farm_reserve_list(c, (size_t)c.capacity / 256)) != MCE_OK) return rc;
    if ((rc = farm_reserve_files(c, 256)) != MCE_OK) return rc;
    MCE_HIP(hipStreamSynchronize(c.stream));
    return MCE_OK;
}

constexpr int64_t kFarmMaxCapacity = (int64_t)1 << 36;
constexpr int32_t kFarmMaxFiles = 1 << 22;

}  // namespace

extern "C" {

int mce_chain_farm_create(int64_t capacity_bytes, int32_t device, void** handle, void** staging)
{
    if (!handle || !staging) return fail(MCE_ERR_INVALID, "chain farm: null pointer argument");
    *handle = nullptr;
    *staging = nullptr;
    if (capacity_bytes < mce::kChainTileBytes || capacity_bytes > kFarmMaxCapacity || capacity_bytes % mce::kChainTileBytes != 0)
        return fail(MCE_ERR_INVALID, "chain farm: a capacity of %lld bytes (a multiple of %lld up to %lld expected)", (long long)capacity_bytes,
                    (long long)mce::kChainTileBytes, (long long)kFarmMaxCapacity);
    int rc = select_device(device);
    if (rc != MCE_OK) return rc;
    FarmDev* c = new FarmDev();
    c->device = device;
    c->capacity = capacity_bytes;
    rc = farm_create(*c);
    if (rc != MCE_OK) {
        delete c;
        return rc;
    }
    c->allocs_wave = 0;
    *handle = c;
    *staging = c->staging;
    return MCE_OK;
}

void mce_chain_farm_destroy(void* handle) { delete static_cast<FarmDev*>(handle); }

int mce_chain_farm_structure(void* handle, const int64_t* file_off, const int64_t* file_len, int32_t nfiles, int64_t wave_bytes, mce_farm_file* files,
                             int64_t* ntok_total)
{
    using namespace mce;
    if (!handle || !file_off || !file_len || !files || !ntok_total) return fail(MCE_ERR_INVALID, "chain farm: null pointer argument");
    if (nfiles < 1 || nfiles > kFarmMaxFiles) return fail(MCE_ERR_INVALID, "chain farm: %d files (1 .. %d expected)", nfiles, kFarmMaxFiles);
    FarmDev& c = *static_cast<FarmDev*>(handle);
    if (wave_bytes > c.capacity || !mce_farm::layout_ok(file_off, file_len, nfiles, wave_bytes))
        return fail(MCE_ERR_INVALID, "chain farm: not a layout of a wave of %lld bytes in a buffer of %lld (offsets on %lld-byte tiles, the first at 0, "
                    "at least one byte behind every file)", (long long)wave_bytes, (long long)c.capacity, (long long)kChainTileBytes);
    *ntok_total = 0;
    int rc = select_device(c.device);
    if (rc != MCE_OK) return rc;
    c.allocs_wave = 0;
    c.ntok = 0;
    c.nfiles = 0;
    if ((rc = farm_reserve_files(c, (size_t)nfiles)) != MCE_OK) return rc;
    const auto t_up = std::chrono::steady_clock::now();
    c.wave_bytes = wave_bytes;
    c.ntiles = wave_bytes / kChainTileBytes;
    const size_t F = c.file_cap + 1;
    int64_t* h_tab = reinterpret_cast<int64_t*>(c.h_small);
    for (int32_t f = 0; f < nfiles; ++f) {
        h_tab[f] = file_off[f];
        h_tab[F + f] = file_len[f];
        h_tab[2 * F + f] = file_off[f] / kChainTileBytes;
    }
    h_tab[nfiles] = wave_bytes;
    h_tab[F + nfiles] = 0;
    h_tab[2 * F + nfiles] = c.ntiles;
    MCE_HIP(hipMemcpyAsync(c.text, c.staging, (size_t)wave_bytes, hipMemcpyHostToDevice, c.stream));          // the whole wave: one copy
    MCE_HIP(hipMemcpyAsync(c.d_ftab, h_tab, 3 * F * sizeof(int64_t), hipMemcpyHostToDevice, c.stream));
    MCE_HIP(hipMemsetAsync(c.tot, 0, sizeof(ChainTotals), c.stream));
    hipLaunchKernelGGL(farm_pad_kernel, dim3(chain_grid(nfiles, 1)), dim3(kChainThreads), 0, c.stream, c.text, c.d_ftab, c.d_ftab + F, (int64_t)nfiles, wave_bytes);
    reader_count_passes(c, c.ntiles);
    MCE_HIP(hipGetLastError());
    ChainTotals* h_tot = reinterpret_cast<ChainTotals*>(c.h_small + 3 * F * sizeof(int64_t));
    mce_farm::FileVerdict* h_files = reinterpret_cast<mce_farm::FileVerdict*>(h_tot + 1);
    MCE_HIP(hipMemcpyAsync(h_tot, c.tot, sizeof(ChainTotals), hipMemcpyDeviceToHost, c.stream));
    MCE_HIP(hipStreamSynchronize(c.stream));
    c.ms_upload = ms_since(t_up);          // (upload, pads and the counting passes: the copy dominates)
    const auto t_st = std::chrono::steady_clock::now();
    const int64_t ntok = (int64_t)h_tot->ntok;
    if (ntok < 0 || ntok > wave_bytes) return fail(MCE_ERR_HIP, "chain farm: %lld tokens in %lld bytes", (long long)ntok, (long long)wave_bytes);
    if ((rc = farm_reserve_tokens(c, (size_t)ntok)) != MCE_OK) return rc;
    if (ntok > 0) reader_token_pass(c, c.ntiles);
    hipLaunchKernelGGL(farm_files_kernel, dim3(chain_grid(nfiles + 1, kChainThreads)), dim3(kChainThreads), 0, c.stream, c.tok_line, c.d_ftab + 2 * F, (int64_t)nfiles,
                       c.tok_base, c.ntiles, c.tot, c.d_files, c.d_ftok0);
    if (ntok > 0)
        hipLaunchKernelGGL(farm_rows_kernel, dim3(chain_grid(ntok, kChainThreads)), dim3(kChainThreads), 0, c.stream, c.tok_line, ntok, c.d_ftok0, (int64_t)nfiles,
                           c.d_files);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(h_files, c.d_files, (size_t)nfiles * sizeof(mce_farm::FileVerdict), hipMemcpyDeviceToHost, c.stream));   // the per-file results: one copy
    MCE_HIP(hipStreamSynchronize(c.stream));
    c.verdicts.assign(h_files, h_files + nfiles);
    int64_t at = 0;
    for (int32_t f = 0; f < nfiles; ++f) {
        const mce_farm::FileVerdict& v = c.verdicts[(size_t)f];
        if (v.tok0 != at || v.ntok < 0 || v.tok0 + v.ntok > ntok)
            return fail(MCE_ERR_HIP, "chain farm: file %d owns the tokens [%lld, %lld + %lld) of %lld", f, (long long)v.tok0, (long long)v.tok0, (long long)v.ntok,
                        (long long)ntok);
        at += v.ntok;
        files[f].tok_base = v.tok0;
        files[f].ntok = v.ntok;
        files[f].ncols = v.ncols;
        files[f].nrows = v.ragged ? 0 : v.nrows;
        files[f].status = v.ragged ? MCE_FARM_RAGGED : MCE_FARM_OK;
        files[f].bad_row = files[f].bad_col = -1;
    }
    if (at != ntok) return fail(MCE_ERR_HIP, "chain farm: the files own %lld of %lld tokens", (long long)at, (long long)ntok);
    c.ntok = ntok;
    c.nfiles = nfiles;
    ++c.waves;
    c.files_total += nfiles;
    c.ms_structure = ms_since(t_st);
    *ntok_total = ntok;
    return MCE_OK;
}

int mce_chain_farm_parse(void* handle, double* d_out, mce_farm_file* files, int32_t nfiles)
{
    using namespace mce;
    if (!handle || !files) return fail(MCE_ERR_INVALID, "chain farm: null pointer argument");
    FarmDev& c = *static_cast<FarmDev*>(handle);
    if (nfiles != c.nfiles || nfiles < 1) return fail(MCE_ERR_INVALID, "chain farm: parse of %d files after a structure pass over %lld", nfiles, (long long)c.nfiles);
    c.ms_parse = c.ms_patch = 0.0;
    c.patched = 0;
    if (c.ntok == 0) return MCE_OK;
    if (!d_out) return fail(MCE_ERR_INVALID, "chain farm: null output buffer");
    int rc = select_device(c.device);
    if (rc != MCE_OK) return rc;
    const auto t_p = std::chrono::steady_clock::now();
    int64_t nlist = 0;
    ChainTotals* h_tot = reinterpret_cast<ChainTotals*>(c.h_small);
    if ((rc = reader_parse(c, "chain farm", c.wave_bytes, c.ntok, d_out, c.list, (int64_t)c.list_cap, false, h_tot, &nlist)) != MCE_OK) return rc;
    if (nlist > (int64_t)c.list_cap) {          // (a wave of nan columns or 25-digit fields: grown once)
        if ((rc = farm_reserve_list(c, (size_t)nlist)) != MCE_OK) return rc;
        if ((rc = reader_parse(c, "chain farm", c.wave_bytes, c.ntok, d_out, c.list, (int64_t)c.list_cap, true, h_tot, &nlist)) != MCE_OK) return rc;
    }
    c.ms_parse = ms_since(t_p);
    if (nlist == 0) return MCE_OK;
    const auto t_d = std::chrono::steady_clock::now();
    std::vector<ChainPatch> patch;          // strtod on the staging bytes (a token holds no pad byte, so these are the file's own)
    std::vector<double> fixed;
    std::vector<size_t> failed;
    if ((rc = reader_host_fixes(c, "chain farm", c.list, nlist, c.ntok, c.wave_bytes, c.staging, patch, fixed, failed)) != MCE_OK) return rc;
    std::vector<int64_t> tok0((size_t)nfiles), bad_tok((size_t)nfiles, -1);
    for (int32_t f = 0; f < nfiles; ++f) tok0[(size_t)f] = c.verdicts[(size_t)f].tok0;
    for (size_t i : failed) {
        const int64_t token = patch[i].token, f = mce_farm::file_of_token(tok0.data(), nfiles, token);
        if (bad_tok[(size_t)f] < 0 || token < bad_tok[(size_t)f]) bad_tok[(size_t)f] = token;
    }
    for (int32_t f = 0; f < nfiles; ++f) {
        if (bad_tok[(size_t)f] < 0 || files[f].status != MCE_FARM_OK || files[f].ncols < 1) continue;
        const int64_t in = bad_tok[(size_t)f] - tok0[(size_t)f];
        files[f].status = MCE_FARM_NOT_A_NUMBER;          // (this file only; row and column are counted inside the file)
        files[f].bad_row = in / files[f].ncols;
        files[f].bad_col = in % files[f].ncols + 1;
    }
    if ((rc = reader_patch(c, c.list, c.fix, fixed, c.ntok, d_out)) != MCE_OK) return rc;
    c.patched = nlist;
    c.ms_patch = ms_since(t_d);
    return MCE_OK;
}

int mce_chain_farm_stats(void* handle, double* stats, int32_t nstats)
{
    if (!handle || !stats || nstats < 12) return fail(MCE_ERR_INVALID, "chain farm: stats[12] expected");
    const FarmDev& c = *static_cast<FarmDev*>(handle);
    const double v[12] = {(double)c.waves, (double)c.files_total, (double)c.allocs, (double)c.allocs_wave, (double)c.grows, (double)c.ntok, (double)c.patched,
                          c.ms_upload, c.ms_structure, c.ms_parse, c.ms_patch, (double)c.capacity};
    std::copy(v, v + 12, stats);
    return MCE_OK;
}

}  // extern "C"

// ---- preparation of the unthinned roots of a wave -------------------------------------------------------------------------------------
namespace {

// the workspace of nroots roots of nparts parts and nrows rows in all.  The tables take 6 (nroots + 1) + 3 nparts words; a root of n
// rows has ceil(n / 512) tiles: at most nrows / 512 + nroots in all
struct FarmPrepWs {
    int64_t* tab;
    double *tile_max, *tile_sumw;
    long long* tile_bad;
    double* red;
    size_t total;
    int64_t ntiles;
    FarmPrepWs(int32_t nroots, int32_t nparts, int64_t nrows, void* ws = nullptr)
    {
        ntiles = nrows / mce::kPrepTile + nroots;
        WsPlan P(ws);
        tab = P.take<int64_t>((size_t)6 * ((size_t)nroots + 1) + (size_t)3 * (size_t)nparts);
        tile_max = P.take<double>((size_t)ntiles);
        tile_sumw = P.take<double>((size_t)ntiles);
        tile_bad = P.take<long long>((size_t)ntiles);
        red = P.take<double>((size_t)nroots * 4);
        total = P.total;
    }
};

constexpr int32_t kFarmMaxRoots = 1 << 20;

}  // namespace

extern "C" {

size_t mce_chain_farm_prep_workspace_bytes(int32_t nroots, int32_t nparts, int64_t nrows)
{
    if (nroots < 1 || nroots > kFarmMaxRoots || nparts < 1 || nparts > kFarmMaxFiles || nrows < 0) return 0;
    return FarmPrepWs(nroots, nparts, nrows).total;
}

int mce_chain_farm_prep_dev(const int32_t* root_nparts, const int64_t* root_ncols, int32_t nroots, const mce_chain_part* parts, int32_t nparts, int32_t iw,
                            int32_t ilike, int32_t itheta, int32_t pos_lnp, double* d_params, double* d_w, double* d_like, double* d_fs, double* out,
                            void* ws, size_t ws_bytes, void* stream)
{
    using namespace mce;
    if (!root_nparts || !root_ncols || !parts || !d_params || !d_w || !d_like || !d_fs || !out || !ws) return fail(MCE_ERR_INVALID, "null pointer argument");
    if (nroots < 1 || nroots > kFarmMaxRoots || nparts < 1 || nparts > kFarmMaxFiles) return fail(MCE_ERR_INVALID, "chain farm prep: %d roots, %d parts", nroots, nparts);
    if (iw < 0 || ilike < 0 || itheta < 0) return fail(MCE_ERR_INVALID, "chain farm prep: columns iw=%d ilike=%d itheta=%d", iw, ilike, itheta);
    std::vector<int64_t> tab;
    const size_t R = (size_t)nroots + 1;
    // row0 | tile0 | part0 | elem0 | param0 | ncols (R each) | part_first | part_rows | part_ptr (nparts each)
    tab.assign(6 * R + 3 * (size_t)nparts, 0);
    int64_t *row0 = tab.data(), *tile0 = row0 + R, *part0 = tile0 + R, *elem0 = part0 + R, *param0 = elem0 + R, *ncols = param0 + R;
    int64_t *part_first = ncols + R, *part_rows = part_first + nparts, *part_ptr = part_rows + nparts;
    int64_t p = 0;
    for (int32_t r = 0; r < nroots; ++r) {
        const int64_t nc = root_ncols[r];
        if (root_nparts[r] < 1 || p + root_nparts[r] > nparts) return fail(MCE_ERR_INVALID, "chain farm prep: root %d has %d parts (of %d in all)", r, root_nparts[r], nparts);
        if (nc <= std::max(iw, std::max(ilike, itheta)) || nc > (1 << 20))
            return fail(MCE_ERR_INVALID, "chain farm prep: columns iw=%d ilike=%d itheta=%d of a root with %lld", iw, ilike, itheta, (long long)nc);
        int64_t n = 0;
        for (int32_t k = 0; k < root_nparts[r]; ++k, ++p) {
            const int rc = prep_check_part("chain farm prep", (long long)p, parts[p]);
            if (rc != MCE_OK) return rc;
            part_first[p] = n;
            part_rows[p] = parts[p].nrows;
            part_ptr[p] = (int64_t)reinterpret_cast<intptr_t>(parts[p].rows);
            n += parts[p].nrows;
        }
        if (n < 1) return fail(MCE_ERR_INVALID, "chain farm prep: root %d has no rows", r);
        ncols[r] = nc;
        row0[r + 1] = row0[r] + n;
        tile0[r + 1] = tile0[r] + (n + kPrepTile - 1) / kPrepTile;
        part0[r + 1] = p;
        elem0[r + 1] = elem0[r] + n * nc;
        param0[r + 1] = param0[r] + n * (nc - itheta);
    }
    if (p != nparts) return fail(MCE_ERR_INVALID, "chain farm prep: the roots own %lld of %d parts", (long long)p, nparts);
    const FarmPrepWs L(nroots, nparts, row0[nroots], ws);
    if (ws_bytes < L.total) return fail(MCE_ERR_WORKSPACE, "chain farm prep: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if (tile0[nroots] > L.ntiles) return fail(MCE_ERR_INVALID, "chain farm prep: %lld tiles, room for %lld", (long long)tile0[nroots], (long long)L.ntiles);
    int rc = prep_need_device();
    if (rc != MCE_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t* const d_tab = L.tab;
    MCE_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    FarmTables t;
    t.row0 = d_tab; t.tile0 = d_tab + R; t.part0 = d_tab + 2 * R; t.elem0 = d_tab + 3 * R; t.param0 = d_tab + 4 * R; t.ncols = d_tab + 5 * R;
    t.part_first = d_tab + 6 * R; t.part_rows = t.part_first + nparts;
    t.part_ptr = reinterpret_cast<const double* const*>(t.part_rows + nparts);
    t.nroots = nroots; t.nparts = nparts;
    double *const tile_max = L.tile_max, *const tile_sumw = L.tile_sumw, *const red = L.red;
    long long* const tile_bad = L.tile_bad;
    hipLaunchKernelGGL(farm_gather_kernel, dim3(prep_grid(elem0[nroots], kPrepThreads)), dim3(kPrepThreads), 0, st, t, iw, ilike, itheta, d_params, d_w, d_like);
    hipLaunchKernelGGL(farm_like_tile_kernel, dim3(prep_grid(tile0[nroots], 1)), dim3(kPrepThreads), 0, st, t, d_like, d_w, pos_lnp ? 1 : 0, tile_max, tile_sumw, tile_bad);
    hipLaunchKernelGGL(farm_like_final_kernel, dim3(prep_grid(nroots, 1)), dim3(kPrepThreads), 0, st, t, tile_max, tile_sumw, tile_bad, red);
    hipLaunchKernelGGL(farm_fs_kernel, dim3(prep_grid(row0[nroots], kPrepThreads)), dim3(kPrepThreads), 0, st, t, d_like, pos_lnp ? 1 : 0, red, d_fs);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, red, (size_t)nroots * 4 * sizeof(double), hipMemcpyDeviceToHost, st));          // every root's scalars: one copy
    MCE_HIP(hipStreamSynchronize(st));
    return MCE_OK;
}

}  // extern "C"
