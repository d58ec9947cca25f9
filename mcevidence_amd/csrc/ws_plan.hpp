// ws_plan.hpp -- the library's workspace planner (host only, plain C++17: the layout headers that a CPU test compiles -- feed_layout.hpp,
// search_layout.hpp -- take it from here, capi.hip through capi_common.hpp).  Still counted by hand with prep_align: the rows of
// capi_prep.hpp and capi_farm.hpp that are not WsPlan takes yet.
#pragma once
#include <cstddef>

inline size_t prep_align(size_t x) { return (x + 255) & ~(size_t)255; }

// a workspace, declared ONCE as a row of take()s: every array starts on a multiple of `align` bytes (256 on the device; a power of
// two).  Over no workspace (ws = null) the row only counts -- `total` is what a *_workspace_bytes function returns --, over a
// workspace it also hands out the typed pointers, so the size and the pointers cannot disagree.
struct WsPlan {
    char* base;
    size_t align, total = 0;
    explicit WsPlan(void* ws, size_t align_ = 256) : base(static_cast<char*>(ws)), align(align_) {}
    char* here() const { return base ? base + total : nullptr; }          // where the next take() starts (a block planned by a row of its own)
    template <class T> T* take(size_t count) { return take_bytes<T>(count * sizeof(T)); }
    template <class T> T* take_bytes(size_t bytes)
    {
        T* const p = reinterpret_cast<T*>(here());
        total += (bytes + align - 1) & ~(align - 1);
        return p;
    }
};
