// capi_chain.hpp -- part of capi.hip (one translation unit): the reader core that the single-file reader (below) and the farm reader
// (capi_farm.hpp) share, and mce_chain_dev_open / _read / _close, chain text -> fp64 on the device (chain_kernels.hpp has the passes).
//
// The core: ReaderDev owns and frees a reader's device scratch; reader_count_passes / reader_token_pass launch the structure passes,
// reader_parse one parse pass, reader_host_fixes downloads and checks the list and runs the host's strtod, reader_patch uploads the
// fixes.  How much is allocated, and when, is each reader's own business.
//
// The single-file reader: open uploads the bytes and runs the structure pass (rows, columns, ragged lines); read runs the parse pass,
// downloads the values and patches the undecided tokens from the CALLER'S buffer -- which therefore must stay valid until close.  Each
// handle has its own stream and scratch (the text, padded to whole tiles; 8 bytes per token of offsets; 8 bytes per token of line
// numbers during open, of values during read; 26 bytes per 4 KB tile), freed in close, and belongs to one thread.
// mce_chain_dev_read_dev leaves the values on the device: the parse pass writes into the caller's device buffer, and the host's
// patches go there in one small copy and one scatter launch (prep_patch_kernel).
#pragma once

#include <chrono>

#include "chain_kernels.hpp"
#include "chain_parse.hpp"
#include "chain_prep_kernels.hpp"

namespace {

// the device scratch every reader has, one file or a wave of files
struct ReaderDev {
    int device = 0;
    hipStream_t stream = nullptr;
    unsigned char* text = nullptr;
    unsigned char *tile_kind = nullptr, *tile_in = nullptr;
    unsigned *tile_ntok = nullptr, *tile_nterm = nullptr;
    unsigned long long *tok_base = nullptr, *term_base = nullptr;
    int64_t *tok_off = nullptr, *tok_line = nullptr;
    uint64_t* pow5 = nullptr;
    mce::ChainTotals* tot = nullptr;
    ~ReaderDev()
    {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (cur != device) (void)hipSetDevice(device);
        for (void* p : {(void*)text, (void*)tile_kind, (void*)tile_in, (void*)tile_ntok, (void*)tile_nterm, (void*)tok_base, (void*)term_base, (void*)tok_off,
                        (void*)tok_line, (void*)pow5, (void*)tot})
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
        if (cur != device) (void)hipSetDevice(cur);
    }
};

struct ChainDev : ReaderDev {
    const char* host_text = nullptr;
    int64_t nbytes = 0, ntiles = 0, ntok = 0, nrows = 0, ncols = 0;
    double ms_upload = 0.0, ms_structure = 0.0;
};

template <class T>
int chain_alloc(T*& p, size_t count, const char* what)
{
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) {
        p = nullptr;
        (void)hipGetLastError();
        return fail(MCE_ERR_HIP, "chain reader: cannot allocate %zu bytes of device memory for %s: %s", count * sizeof(T), what, hipGetErrorString(e));
    }
    return MCE_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// blocks for `items` at `per_block` each, at most `blocks_per_cu` per compute unit (the kernels' loops stride over the rest)
unsigned grid_for(int64_t items, int64_t per_block, int blocks_per_cu)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per_block - 1) / per_block, (int64_t)kAssumedCUs * blocks_per_cu));
}
unsigned chain_grid(int64_t items, int64_t per_block) { return grid_for(items, per_block, 64); }
unsigned prep_grid(int64_t items, int64_t per_block) { return grid_for(items, per_block, 16); }

// the counting passes over `ntiles` tiles of c.text: comment states, token and line-end counts, their exclusive sums, c.tot->ntok / nterm
void reader_count_passes(const ReaderDev& c, int64_t ntiles)
{
    using namespace mce;
    const unsigned grid = chain_grid(ntiles, 1);
    hipLaunchKernelGGL(chain_tile_kernel<0>, dim3(grid), dim3(kChainThreads), 0, c.stream, c.text, ntiles, c.tile_kind, c.tile_in, c.tile_ntok, c.tile_nterm,
                       c.tok_base, c.term_base, (int64_t*)nullptr, (int64_t*)nullptr);
    hipLaunchKernelGGL(chain_scan_state_kernel, dim3(1), dim3(kChainScanThreads), 0, c.stream, c.tile_kind, ntiles, c.tile_in);
    hipLaunchKernelGGL(chain_tile_kernel<1>, dim3(grid), dim3(kChainThreads), 0, c.stream, c.text, ntiles, c.tile_kind, c.tile_in, c.tile_ntok, c.tile_nterm,
                       c.tok_base, c.term_base, (int64_t*)nullptr, (int64_t*)nullptr);
    hipLaunchKernelGGL(chain_scan_count_kernel, dim3(1), dim3(kChainScanThreads), 0, c.stream, c.tile_ntok, c.tile_nterm, ntiles, c.tok_base, c.term_base, c.tot);
}

// the token pass: c.tok_off / c.tok_line of every token (both hold at least the counted tokens)
void reader_token_pass(const ReaderDev& c, int64_t ntiles)
{
    using namespace mce;
    hipLaunchKernelGGL(chain_tile_kernel<2>, dim3(chain_grid(ntiles, 1)), dim3(kChainThreads), 0, c.stream, c.text, ntiles, c.tile_kind, c.tile_in, c.tile_ntok,
                       c.tile_nterm, c.tok_base, c.term_base, c.tok_off, c.tok_line);
}

// One parse pass: `ntok` tokens of the `nbytes` of c.text -> d_vals, the undecided ones -> list[cap]; *nlist counts them.  More than
// cap: the reader grows the list and calls again with `second` set (a text of nan columns or 25-digit fields).
int reader_parse(const ReaderDev& c, const char* who, int64_t nbytes, int64_t ntok, double* d_vals, mce::ChainPatch* list, int64_t cap, bool second,
                 mce::ChainTotals* h_tot, int64_t* nlist)
{
    using namespace mce;
    MCE_HIP(hipMemsetAsync(&c.tot->nlist, 0, sizeof(unsigned long long), c.stream));
    hipLaunchKernelGGL(chain_parse_kernel, dim3(chain_grid(ntok, kChainThreads)), dim3(kChainThreads), 0, c.stream, reinterpret_cast<const char*>(c.text), nbytes,
                       c.tok_off, ntok, c.pow5, d_vals, list, cap, c.tot);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(h_tot, c.tot, sizeof(ChainTotals), hipMemcpyDeviceToHost, c.stream));
    MCE_HIP(hipStreamSynchronize(c.stream));
    *nlist = (int64_t)h_tot->nlist;
    if (second && *nlist > cap)
        return fail(MCE_ERR_HIP, "%s: the list of undecided tokens changed between two passes (%lld > %lld)", who, (long long)*nlist, (long long)cap);
    return MCE_OK;
}

// The host fix-up: the list comes down (with whatever the caller queued before; *synced: when), every entry is checked against `ntok`
// tokens in `nbytes` bytes, strtod runs on `host_text`: fixed[i] for patch[i], NaN and i in `failed` where the host refuses it too.
int reader_host_fixes(const ReaderDev& c, const char* who, const mce::ChainPatch* list, int64_t nlist, int64_t ntok, int64_t nbytes, const char* host_text,
                      std::vector<mce::ChainPatch>& patch, std::vector<double>& fixed, std::vector<size_t>& failed,
                      std::chrono::steady_clock::time_point* synced = nullptr)
{
    patch.resize((size_t)nlist);
    fixed.resize((size_t)nlist);
    if (nlist > 0) MCE_HIP(hipMemcpyAsync(patch.data(), list, (size_t)nlist * sizeof(mce::ChainPatch), hipMemcpyDeviceToHost, c.stream));
    MCE_HIP(hipStreamSynchronize(c.stream));
    if (synced) *synced = std::chrono::steady_clock::now();
    for (size_t i = 0; i < patch.size(); ++i) {
        const mce::ChainPatch& p = patch[i];
        if (p.token < 0 || p.token >= ntok || p.offset < 0 || p.length < 0 || p.offset + p.length > nbytes)
            return fail(MCE_ERR_HIP, "%s: a listed token lies outside the text (token %lld, offset %lld, length %lld)", who, (long long)p.token, (long long)p.offset,
                        (long long)p.length);
        if (!mce_parse::parse_slow(host_text + p.offset, host_text + p.offset + p.length, &fixed[i])) {
            fixed[i] = std::nan("");
            failed.push_back(i);
        }
    }
    return MCE_OK;
}

// the fixes go up into `fix` and from there into d_vals[token]
int reader_patch(const ReaderDev& c, const mce::ChainPatch* list, double* fix, const std::vector<double>& fixed, int64_t ntok, double* d_vals)
{
    const int64_t nlist = (int64_t)fixed.size();
    MCE_HIP(hipMemcpyAsync(fix, fixed.data(), (size_t)nlist * sizeof(double), hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(mce::prep_patch_kernel, dim3(chain_grid(nlist, mce::kPrepThreads)), dim3(mce::kPrepThreads), 0, c.stream, list, fix, nlist, ntok, d_vals);
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipStreamSynchronize(c.stream));
    return MCE_OK;
}

int chain_dev_structure(ChainDev& c)
{
    using namespace mce;
    const auto t_up = std::chrono::steady_clock::now();
    c.ntiles = (c.nbytes + kChainTileBytes - 1) / kChainTileBytes;
    const size_t padded = (size_t)c.ntiles * (size_t)kChainTileBytes;
    int rc;
    if ((rc = chain_alloc(c.text, padded, "the text")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.tot, 1, "the totals")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.pow5, (size_t)mce_parse::kPow5Words, "the powers of five")) != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(c.text, c.host_text, (size_t)c.nbytes, hipMemcpyHostToDevice, c.stream));
    if (padded > (size_t)c.nbytes) MCE_HIP(hipMemsetAsync(c.text + c.nbytes, '\n', padded - (size_t)c.nbytes, c.stream));
    MCE_HIP(hipMemsetAsync(c.tot, 0, sizeof(ChainTotals), c.stream));
    MCE_HIP(hipMemcpyAsync(c.pow5, mce_parse::pow5_table(), (size_t)mce_parse::kPow5Words * sizeof(uint64_t), hipMemcpyHostToDevice, c.stream));
    MCE_HIP(hipStreamSynchronize(c.stream));
    c.ms_upload = ms_since(t_up);

    const auto t_st = std::chrono::steady_clock::now();
    const size_t nt = (size_t)c.ntiles;
    if ((rc = chain_alloc(c.tile_kind, nt, "the tile states")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.tile_in, nt, "the tile states")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.tile_ntok, nt, "the tile counts")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.tile_nterm, nt, "the tile counts")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.tok_base, nt, "the tile offsets")) != MCE_OK) return rc;
    if ((rc = chain_alloc(c.term_base, nt, "the tile offsets")) != MCE_OK) return rc;
    reader_count_passes(c, c.ntiles);
    MCE_HIP(hipGetLastError());
    ChainTotals tot;
    MCE_HIP(hipMemcpyAsync(&tot, c.tot, sizeof(tot), hipMemcpyDeviceToHost, c.stream));
    MCE_HIP(hipStreamSynchronize(c.stream));
    c.ntok = (int64_t)tot.ntok;
    if (c.ntok > 0) {
        if ((rc = chain_alloc(c.tok_off, (size_t)c.ntok, "the token offsets")) != MCE_OK) return rc;
        if ((rc = chain_alloc(c.tok_line, (size_t)c.ntok, "the token lines")) != MCE_OK) return rc;
        reader_token_pass(c, c.ntiles);
        hipLaunchKernelGGL(chain_ncols_kernel, dim3(1), dim3(64), 0, c.stream, c.tok_line, c.tot);
        hipLaunchKernelGGL(chain_rows_kernel, dim3(chain_grid(c.ntok, kChainThreads)), dim3(kChainThreads), 0, c.stream, c.tok_line, c.tot);
        MCE_HIP(hipGetLastError());
        MCE_HIP(hipMemcpyAsync(&tot, c.tot, sizeof(tot), hipMemcpyDeviceToHost, c.stream));
        MCE_HIP(hipStreamSynchronize(c.stream));
        MCE_HIP(hipFree(c.tok_line));          // (only the structure check reads the line numbers)
        c.tok_line = nullptr;
        c.ncols = (int64_t)tot.ncols;
        if (tot.ragged || c.ncols < 1 || c.ntok % c.ncols != 0)
            return fail(MCE_ERR_INVALID, "chain reader: the number of columns changed: not every data line holds the %lld fields of the first one", (long long)c.ncols);
        c.nrows = c.ntok / c.ncols;
    }
    c.ms_structure = ms_since(t_st);
    return MCE_OK;
}

}  // namespace

extern "C" {

int mce_chain_dev_open(const char* text, int64_t nbytes, int32_t device, void** handle, int64_t* nrows, int64_t* ncols)
{
    if (!handle || !nrows || !ncols || nbytes < 0 || (!text && nbytes > 0)) return fail(MCE_ERR_INVALID, "chain reader: null pointer or negative size");
    *handle = nullptr;
    *nrows = *ncols = 0;
    int rc = select_device(device);
    if (rc != MCE_OK) return rc;
    ChainDev* c = new ChainDev();
    c->device = device;
    c->host_text = text;
    c->nbytes = nbytes;
    if (nbytes > 0) {
        const hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            c->stream = nullptr;
            delete c;
            return fail(MCE_ERR_HIP, "chain reader: hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
        }
        rc = chain_dev_structure(*c);
        if (rc != MCE_OK) {
            delete c;
            return rc;
        }
    }
    *nrows = c->nrows;
    *ncols = c->ncols;
    *handle = c;
    return MCE_OK;
}

}  // extern "C"

namespace {

// out: host memory (out_device false: the values are downloaded and patched there) or device memory on the handle's device
int chain_dev_read_impl(void* handle, double* out, bool out_device, double* stats, int32_t nstats)
{
    using namespace mce;
    if (!handle) return fail(MCE_ERR_INVALID, "chain reader: null handle");
    ChainDev& c = *static_cast<ChainDev*>(handle);
    if (stats && nstats < 6) return fail(MCE_ERR_INVALID, "chain reader: stats[6] expected");
    double ms_parse = 0.0, ms_down = 0.0;
    int64_t npatched = 0;
    if (c.ntok > 0) {
        if (!out) return fail(MCE_ERR_INVALID, "chain reader: null output buffer");
        int rc = select_device(c.device);
        if (rc != MCE_OK) return rc;
        const auto t_p = std::chrono::steady_clock::now();
        struct Scratch {
            double *vals = nullptr, *fix = nullptr;
            ChainPatch* list = nullptr;
            ~Scratch() { if (vals) (void)hipFree(vals); if (fix) (void)hipFree(fix); if (list) (void)hipFree(list); }
        } s;
        if (!out_device && (rc = chain_alloc(s.vals, (size_t)c.ntok, "the values")) != MCE_OK) return rc;
        double* const d_vals = out_device ? out : s.vals;
        // the undecided tokens: room for one token in 32 at first; a file that needs more gets a list of the counted size and a second pass
        int64_t cap = std::max<int64_t>(4096, c.ntok / 32), nlist = 0;
        ChainTotals tot;
        if ((rc = chain_alloc(s.list, (size_t)cap, "the list of undecided tokens")) != MCE_OK) return rc;
        if ((rc = reader_parse(c, "chain reader", c.nbytes, c.ntok, d_vals, s.list, cap, false, &tot, &nlist)) != MCE_OK) return rc;
        if (nlist > cap) {
            MCE_HIP(hipFree(s.list));
            s.list = nullptr;
            cap = nlist;
            if ((rc = chain_alloc(s.list, (size_t)cap, "the list of undecided tokens")) != MCE_OK) return rc;
            if ((rc = reader_parse(c, "chain reader", c.nbytes, c.ntok, d_vals, s.list, cap, true, &tot, &nlist)) != MCE_OK) return rc;
        }
        ms_parse = ms_since(t_p);
        const auto t_d = std::chrono::steady_clock::now();
        auto synced = t_d;
        if (!out_device) MCE_HIP(hipMemcpyAsync(out, s.vals, (size_t)c.ntok * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        std::vector<ChainPatch> patch;          // host fix-up: strtod on the caller's own bytes
        std::vector<double> fixed;
        std::vector<size_t> failed;
        if ((rc = reader_host_fixes(c, "chain reader", s.list, nlist, c.ntok, c.nbytes, c.host_text, patch, fixed, failed, &synced)) != MCE_OK) return rc;
        ms_down = std::chrono::duration<double, std::milli>(synced - t_d).count();
        npatched = nlist;
        if (!failed.empty()) {
            const ChainPatch* bad = &patch[failed[0]];          // the lowest token: the list is in no order
            for (size_t i : failed)
                if (patch[i].token < bad->token) bad = &patch[i];
            return fail(MCE_ERR_INVALID, "could not convert string '%.*s' to float64 at row %lld, column %lld", (int)std::min<int64_t>(bad->length, 60),
                        c.host_text + bad->offset, (long long)(bad->token / c.ncols), (long long)(bad->token % c.ncols + 1));
        }
        if (!out_device)
            for (size_t i = 0; i < patch.size(); ++i) out[patch[i].token] = fixed[i];
        else if (nlist > 0) {
            if ((rc = chain_alloc(s.fix, (size_t)nlist, "the patched values")) != MCE_OK) return rc;
            if ((rc = reader_patch(c, s.list, s.fix, fixed, c.ntok, d_vals)) != MCE_OK) return rc;
            ms_down = ms_since(t_d);
        }
    }
    if (stats) {
        stats[0] = (double)c.ntok;
        stats[1] = (double)npatched;
        stats[2] = c.ms_upload;
        stats[3] = c.ms_structure;
        stats[4] = ms_parse;
        stats[5] = ms_down;
    }
    return MCE_OK;
}

}  // namespace

extern "C" {

int mce_chain_dev_read(void* handle, double* out, double* stats, int32_t nstats) { return chain_dev_read_impl(handle, out, false, stats, nstats); }

int mce_chain_dev_read_dev(void* handle, double* d_out, double* stats, int32_t nstats) { return chain_dev_read_impl(handle, d_out, true, stats, nstats); }

void mce_chain_dev_close(void* handle) { delete static_cast<ChainDev*>(handle); }

}  // extern "C"
