// agt_side_buffers.h -- the device buffers of a side library's handle: one stream, the allocations made on it, synchronous copies.
// Every function returns one of agt_side_math.h's codes, which are the library's own (0, *_ERR_ALLOC, *_ERR_HIP).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "agt_side_math.h"

#define HC(call) do { if ((call) != hipSuccess) { (void)hipGetLastError(); return agt_side::ERR_HIP; } } while (0)
#define RC(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

struct AgtSideBuffers {
    hipStream_t stream = nullptr;
    std::vector<void*> allocs;

    // (a size of zero still yields a pointer of its own: 8 bytes)
    int alloc(void** p, size_t bytes)
    {
        if (hipMalloc(p, bytes ? bytes : 8) != hipSuccess) { (void)hipGetLastError(); return agt_side::ERR_ALLOC; }
        allocs.push_back(*p);
        return agt_side::OK;
    }

    template <class T>
    int alloc_n(T** p, size_t count) { return alloc(reinterpret_cast<void**>(p), count * sizeof(T)); }

    int upload(void* dst, const void* src, size_t bytes)
    {
        if (!bytes) return agt_side::OK;
        HC(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
        HC(hipStreamSynchronize(stream));             // (the source is the caller's or a local: it must be read before this returns)
        return agt_side::OK;
    }

    // (a NULL destination is an output the caller did not ask for)
    int download(void* dst, const void* src, size_t bytes)
    {
        if (!bytes || !dst) return agt_side::OK;
        HC(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
        HC(hipStreamSynchronize(stream));
        return agt_side::OK;
    }

    void free_all()
    {
        for (void* p : allocs) (void)hipFree(p);
        allocs.clear();
    }
};

// the end of a handle made with new whose device memory is all in its member `buf`: also the way out of a create that failed half-way
template <class Handle>
int agt_side_destroy(Handle* h)
{
    if (!h) return agt_side::ERR_ARG;
    h->buf.free_all();
    delete h;
    return agt_side::OK;
}
