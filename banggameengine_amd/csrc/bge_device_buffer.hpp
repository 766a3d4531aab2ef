// bge_device_buffer.hpp — the one owner of the library's device and page-locked memory.
//
// A Buffer frees its block when it dies, moves (std::swap works) and cannot be copied, so a buffer that is a member or a local
// needs its declaration and nothing else.  ensure() is grow-only; an ensure that grows frees the old block FIRST and does not
// keep its contents.  The allocator A is the seam: `error`, `ok`, alloc(void**, size_t) and free(void*).  The library uses the
// two HIP allocators at the end of this file; without HIP on the include path only the template exists (tests/cpp/device_buffer.cpp
// runs it over a counting stand-in).
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace bge {

// Blocks and bytes held by live Buffers of this process, of every allocator (bge_device_memory): one relaxed add per allocation.
struct LiveMemory {
    std::atomic<uint64_t> allocations{0}, bytes{0};
};
inline LiveMemory& live_memory()
{
    static LiveMemory m;
    return m;
}

template <class A> struct Buffer {
    void* p = nullptr;
    size_t bytes = 0;
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept
    {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~Buffer() { release(); }
    typename A::error ensure(size_t need)
    {
        if (need <= bytes) return A::ok;
        release();
        const typename A::error e = A::alloc(&p, need);
        if (e != A::ok) {
            p = nullptr;
            return e;
        }
        bytes = need;
        live_memory().allocations.fetch_add(1, std::memory_order_relaxed);
        live_memory().bytes.fetch_add(need, std::memory_order_relaxed);
        return e;
    }
    void release()
    {
        if (!p) return;
        A::free(p);
        live_memory().allocations.fetch_sub(1, std::memory_order_relaxed);
        live_memory().bytes.fetch_sub(bytes, std::memory_order_relaxed);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

} // namespace bge

#if __has_include(<hip/hip_runtime_api.h>)
#include <hip/hip_runtime_api.h>

namespace bge {

struct HipDeviceMemory {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void** p, size_t n) { return hipMalloc(p, n); }
    static void free(void* p) { (void)hipFree(p); }
};
struct HipPinnedMemory {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static void free(void* p) { (void)hipHostFree(p); }
};
using DevBuf = Buffer<HipDeviceMemory>;
using PinnedBuf = Buffer<HipPinnedMemory>;

} // namespace bge
#endif
