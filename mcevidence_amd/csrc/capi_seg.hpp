// capi_seg.hpp -- part of capi.hip (one translation unit): what the host sides of the segment-tile families (capi_moments.hpp,
// capi_jackres.hpp, capi_summary.hpp, capi_cov.hpp, capi_kde.hpp, capi_marginals.hpp, capi_contours.hpp; the scheme: seg_tiles.hpp)
// share: the opening and the end of their _dev forms and the staging of their host-pointer forms.  Each family keeps its own argument
// checks and error texts.  (What the four families that begin with summary's moments share beyond this: capi_sum_front.hpp.)
#pragma once

#include "seg_tiles.hpp"

namespace {

// the opening of a _dev form, after the argument checks: the workspace holds the plan, a device is there, and the segment table and the
// first tiles are on their way to it
template <class Seg>
int seg_dev_begin(const char* who, size_t ws_bytes, size_t need, const std::vector<Seg>& table, const std::vector<int64_t>& tile0, Seg* d_segs, int64_t* d_tile0,
                  hipStream_t st)
{
    if (ws_bytes < need) return fail(MCE_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    const int rc = prep_need_device();
    if (rc != MCE_OK) return rc;
    MCE_HIP(hipMemcpyAsync(d_segs, table.data(), table.size() * sizeof(Seg), hipMemcpyHostToDevice, st));
    MCE_HIP(hipMemcpyAsync(d_tile0, tile0.data(), tile0.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return MCE_OK;
}

// the end of a _dev form, after its last launch: the launches went through, and the block of results is with the caller
int seg_dev_end(double* out, const double* res, size_t doubles, hipStream_t st)
{
    MCE_HIP(hipGetLastError());
    MCE_HIP(hipMemcpyAsync(out, res, doubles * 8, hipMemcpyDeviceToHost, st));
    MCE_HIP(hipStreamSynchronize(st));                            // the one wait
    return MCE_OK;
}

// kernels that stage more LDS than the default limit: raise it once per device (attr_set: the family's flags; a failure is not
// remembered: the next call asks again)
struct SegLdsAttr {
    const void* kernel;
    size_t bytes;
};
int seg_attr_once(std::atomic<bool> (&attr_set)[kMaxDevices], std::initializer_list<SegLdsAttr> list)
{
    int dev = 0;
    MCE_HIP(hipGetDevice(&dev));
    if (dev >= kMaxDevices || !attr_set[dev].load()) {
        for (const SegLdsAttr& a : list) MCE_HIP(hipFuncSetAttribute(a.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.bytes));
        if (dev < kMaxDevices) attr_set[dev].store(true);
    }
    return MCE_OK;
}

// a host-pointer form stages the columns of all its segments in ONE device buffer, one behind the other, and hands the device form
// their addresses: alloc() the bytes of all columns (seg_stage_bytes each), then put() them in any order
size_t seg_stage_bytes(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

struct SegStage {
    DevBuf buf;
    char* at = nullptr;
    int alloc(size_t bytes)
    {
        MCE_HIP(buf.alloc(bytes));
        at = buf.as<char>();
        return MCE_OK;
    }
    // `rows` rows of `width` values of T, `ld` values apart on the host (null, or no rows: no column) -> packed on the device; dev:
    // its address there (null)
    template <class T> int put(const T* src, size_t rows, const T*& dev, size_t width = 1, size_t ld = 1)
    {
        dev = nullptr;
        if (!src || rows == 0) return MCE_OK;
        if (ld == width) MCE_HIP(hipMemcpy(at, src, rows * width * sizeof(T), hipMemcpyHostToDevice));
        else MCE_HIP(hipMemcpy2D(at, width * sizeof(T), src, ld * sizeof(T), width * sizeof(T), rows, hipMemcpyHostToDevice));
        dev = reinterpret_cast<const T*>(at);
        at += seg_stage_bytes(rows * width * sizeof(T));
        return MCE_OK;
    }
};

// the staging of a host-pointer form whose segments are (x, ld, n, d, w): of every segment the d measured columns packed (ld = d on the
// device), then the weights, in one buffer of `data`; dsegs: the segments at their device addresses
template <class Seg> int seg_stage_xw(const Seg* segs, int32_t nseg, SegStage& data, std::vector<Seg>& dsegs)
{
    size_t elems = 0;
    for (int32_t s = 0; s < nseg; ++s) elems += (size_t)segs[s].n * ((size_t)segs[s].d + 1);
    int rc = data.alloc(elems * sizeof(double));
    if (rc != MCE_OK) return rc;
    dsegs.assign(segs, segs + nseg);
    for (Seg& g : dsegs) {
        if ((rc = data.put(g.x, (size_t)g.n, g.x, (size_t)g.d, (size_t)g.ld)) != MCE_OK || (rc = data.put(g.w, (size_t)g.n, g.w)) != MCE_OK) return rc;
        g.ld = g.d;
    }
    return MCE_OK;
}

}  // namespace
