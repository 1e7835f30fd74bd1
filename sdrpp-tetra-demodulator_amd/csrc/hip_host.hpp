// hip_host.hpp -- host-side plumbing shared by the C ABI sources (no device code): the device guard, the HIP status checks and
// move-only owners of device memory, page-locked host memory, streams and events.  An owner converts implicitly to its raw
// handle, so kernel arguments and hipMemcpy calls take it as they are; it releases what it holds when it goes out of scope.
// DelayLine (at the end) is the two-buffer delay line of the streaming stages (channeliser, resampler) with its carry rule.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

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

// The delay line of a streaming stage: the `rows` newest rows (row_elems elements of T each) before the next call's first, held
// in one of two device buffers.  The carry rule, once: after a call of n_in rows the last `rows` of [delay line | new] become the
// line -- written into the OTHER buffer (an in-place move would overlap for n_in < rows), then the two swap roles: keep = rows -
// min(n_in, rows) rows come from the old line, the from_x = min(n_in, rows) newest input rows behind them.  All copies go to the
// caller's stream: its order keeps the call's kernel ahead of them and them ahead of the next call's writes.
template <class T> class DelayLine {
public:
    // tail_elems: room behind the line in both buffers, for a stage that stages the call's rows there ([line | new])
    hipError_t reserve(size_t rows, size_t row_elems, size_t tail_elems = 0) {
        rows_ = rows; row_ = row_elems;
        const hipError_t e = cur_.reserve(sizeof(T) * (rows * row_elems + tail_elems));
        return e != hipSuccess ? e : alt_.reserve(sizeof(T) * (rows * row_elems + tail_elems));
    }
    hipError_t reset() { return hipMemset(cur_, 0, sizeof(T) * rows_ * row_); }
    // the same on the stage's stream, behind the calls enqueued there and ahead of the next
    hipError_t reset_on(hipStream_t s) { return hipMemsetAsync(cur_, 0, sizeof(T) * rows_ * row_, s); }
    operator T*() const { return cur_; }
    T* get() const { return cur_.get(); }
    // copy_new(dst, from_x) copies the from_x newest input rows to dst and returns its hipError_t.
    template <class CopyNew> hipError_t carry(size_t n_in, hipStream_t s, CopyNew copy_new) {
        if (n_in == 0) return hipSuccess;
        const size_t from_x = n_in < rows_ ? n_in : rows_, keep = rows_ - from_x;
        hipError_t e = keep ? hipMemcpyAsync(alt_, cur_ + n_in * row_, sizeof(T) * keep * row_, hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess) e = copy_new(alt_ + keep * row_, from_x);
        if (e == hipSuccess) std::swap(cur_, alt_);
        return e;
    }
    // The same for a stage whose new rows already lie behind the line in this buffer: both parts are one contiguous run.
    hipError_t carry_staged(size_t n_in, hipStream_t s) {
        if (n_in == 0) return hipSuccess;
        const hipError_t e = hipMemcpyAsync(alt_, cur_ + n_in * row_, sizeof(T) * rows_ * row_, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) std::swap(cur_, alt_);
        return e;
    }

private:
    DevMem<T> cur_, alt_;
    size_t rows_ = 0, row_ = 0;
};
