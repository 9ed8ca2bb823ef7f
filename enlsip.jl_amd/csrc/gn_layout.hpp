// Workspace layouts: one description yields both the byte count and the pointers.  Host-only, nothing of HIP.
// A layout is a struct of pointers with `void carve(gn::Carver& c, <shape>)` that asks for its arrays in order.  The same
// function runs twice: on a Carver without a base it only adds up (bytes()), on one with the grown buffer's base it hands out
// the pointers.  Nothing else knows a size, so no call site carries a slack constant.
#pragma once
#include <cstddef>
#include <vector>

namespace gn {

struct Carver {
    struct Entry { const char* name; size_t offset, bytes, align; };
    char* base = nullptr;                  // nullptr: measuring pass
    size_t off = 0;                        // end of the last array = bytes needed so far
    std::vector<Entry>* trace = nullptr;   // set by the layout test: every request, in order

    // `count` elements of T at the next multiple of `align` bytes (a power of two the buffer's base satisfies)
    template <class T>
    void take(T*& ptr, const char* name, size_t count, size_t align = alignof(T)) {
        ptr = (T*)raw(name, count * sizeof(T), align);
    }
    // the same for a type this header cannot name (device records): `bytes` bytes
    void* raw(const char* name, size_t bytes, size_t align) {
        off = (off + align - 1) / align * align;
        if (trace) trace->push_back({name, off, bytes, align});
        void* r = base ? base + off : nullptr;
        off += bytes;
        return r;
    }
    size_t bytes() const { return off; }
};

// bytes a layout needs for this shape
template <class Layout, class... Shape>
size_t layout_bytes(const Shape&... shape) {
    Layout probe;
    Carver c;
    probe.carve(c, shape...);
    return c.bytes();
}

// Measure, grow, place: `grow(bytes)` returns 0 and the buffer's base through its argument, or an error code.
template <class Layout, class Grow, class... Shape>
int place(Layout& L, Grow&& grow, const Shape&... shape) {
    void* base = nullptr;
    const int rc = grow(layout_bytes<Layout>(shape...), &base);
    if (rc) return rc;
    Carver c;
    c.base = (char*)base;
    L.carve(c, shape...);
    return 0;
}

}  // namespace gn
