// The arrays of a host call as one block (free of HIP: plain g++ compiles it, tests/cpp/stage_driver.cpp).  A host entry add()s its
// input arrays in order, copy()s them into the pinned staging buffer and sends that up with one DMA; at() is a part's address in the
// device copy.  The outputs are a second Block of add(nullptr, n) parts: at() then addresses the device block and the pinned block
// the results come back in.  Every part begins on a 16-byte boundary.  matcher_handle.hpp has the steps that touch the handle.
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

namespace snk
{
inline size_t align16(size_t x)
{
    return (x + 15) & ~(size_t)15;
}

struct Block
{
    struct Part
    {
        const void* src;
        size_t bytes, offset;
    };
    std::vector<Part> parts;
    size_t bytes = 0;  // every part padded to 16: the size of the upload
    int add(const void* src, size_t n)
    {
        parts.push_back(Part{src, n, bytes});
        bytes += align16(n);
        return (int)parts.size() - 1;
    }
    // the parts that have a source, into host[0 .. bytes); the padding and the parts without one are left as they are
    void copy(char* host) const
    {
        for (const Part& p : parts)
            if (p.bytes && p.src) memcpy(host + p.offset, p.src, p.bytes);
    }
    template <class T>
    T* at(char* base, int part) const
    {
        return reinterpret_cast<T*>(base + parts[(size_t)part].offset);
    }
    // the last part's end without its padding: what a result block has to hold
    size_t end() const { return parts.empty() ? 0 : parts.back().offset + parts.back().bytes; }
};
}  // namespace snk
