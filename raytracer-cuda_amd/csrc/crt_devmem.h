// crt_devmem.h — the owners of device memory, pinned host memory and HIP events (host code only).
// Everything the library allocates on a device is held by one of these types, so it is released when its handle, its
// state struct or its scope ends, on every return path.  No pooling and no caching: each call is the HIP call.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <utility>

// Live DevBuf / PinnedBuf allocations of the process and their bytes (crt_debug_live_allocations): a test's way to
// see that a sequence of calls released what it allocated, independent of what else runs on the device.
inline std::atomic<int64_t> g_live_buffers{0}, g_live_bytes{0};

// Move-only owner of `size()` elements of T: device memory, or pinned host memory with PINNED.
template <class T, bool PINNED = false>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~DevBuf() { reset(); }

    // Releases what is held, then allocates max(count, 1) elements.  On failure the buffer is empty.
    hipError_t alloc(size_t count) {
        reset();
        if (count < 1) count = 1;
        void* p = nullptr;
        const hipError_t e = PINNED ? hipHostMalloc(&p, count * sizeof(T)) : hipMalloc(&p, count * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); n_ = count;
        ++g_live_buffers; g_live_bytes += (int64_t)(n_ * sizeof(T));
        return hipSuccess;
    }
    // At least `count` elements: nothing when they are there, else alloc (the contents are not kept).
    hipError_t grow(size_t count) { return count <= n_ ? hipSuccess : alloc(count); }
    void reset() {
        if (!p_) return;
        (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        --g_live_buffers; g_live_bytes -= (int64_t)(n_ * sizeof(T));
        p_ = nullptr; n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T>
using PinnedBuf = DevBuf<T, true>;

// Move-only owner of one HIP event.
class DevEvent {
public:
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    DevEvent& operator=(DevEvent&& o) noexcept { std::swap(e_, o.e_); return *this; }
    ~DevEvent() { if (e_) (void)hipEventDestroy(e_); }
    hipError_t create() { return e_ ? hipSuccess : hipEventCreate(&e_); }
    hipEvent_t get() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};
