// hip_host.hpp -- host-side plumbing shared by the C ABI sources (no device code): the device guard, the HIP status checks and
// move-only owners of device memory, page-locked host memory, streams and events.  An owner converts implicitly to its raw
// handle, so kernel arguments and hipMemcpy calls take it as they are; it releases what it holds when it goes out of scope.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

// Selects `dev` for the scope (a negative one keeps the current device) and restores the caller's device on exit.
struct DeviceGuard {
    int prev = -1;
    bool ok;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = dev < 0 || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// A failed HIP call: its status goes to h->last_hip and the entry point returns TETRA_ERR_HIP.
#define HIP_TRY(h, expr)                                  \
    do {                                                  \
        const hipError_t e__ = (expr);                    \
        if (e__ != hipSuccess) {                          \
            (h)->last_hip = (int)e__;                     \
            return TETRA_ERR_HIP;                         \
        }                                                 \
    } while (0)
// A TETRA_* status other than TETRA_OK is returned as it is.
#define TETRA_TRY(expr)                                   \
    do {                                                  \
        const int rc__ = (expr);                          \
        if (rc__ != TETRA_OK) return rc__;                \
    } while (0)

// Owner of one HIP handle (or library handle) H, released with Destroy.  put() releases what it holds and hands out the
// address for a create call to fill.
template <class H, auto Destroy> class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Handle() { reset(); }
    operator H() const { return h_; }
    H* put() { reset(); return &h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

// Owner of one block of device memory (Pinned = false: hipMalloc / hipFree) or page-locked host memory (Pinned = true:
// hipHostMalloc / hipHostFree), typed T*, that knows its capacity in bytes.
template <class T, bool Pinned> class Mem {
public:
    Mem() = default;
    Mem(Mem&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Mem& operator=(Mem&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~Mem() { reset(); }
    operator T*() const { return p_; }
    T* get() const { return p_; }          // for casts, which do not look for the conversion
    size_t bytes() const { return bytes_; }
    // Capacity of at least `n` bytes.  A block that is too small is freed BEFORE the new one is allocated (never two at once);
    // on failure the owner is empty.  host_flags: hipHostMalloc's flags (page-locked memory only).
    hipError_t reserve(size_t n, unsigned host_flags = hipHostMallocDefault) {
        if (n <= bytes_) return hipSuccess;
        reset();
        void* p = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&p, n, host_flags) : hipMalloc(&p, n);
        if (e == hipSuccess) { p_ = static_cast<T*>(p); bytes_ = n; }
        return e;
    }
    T* release() {
        T* p = p_;
        p_ = nullptr; bytes_ = 0;
        return p;
    }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; bytes_ = 0;
    }

private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
};
template <class T> using DevMem = Mem<T, false>;
template <class T> using HostMem = Mem<T, true>;
