// retune_list.hpp -- short host lists (channel indices, bins) on their way to the device without a host synchronisation: a ring of
// page-locked staging blocks with a device copy each.  The caller's list is copied into a block at once (the call may return before
// the device has read it); the block is reused after kSlots - 1 later lists, and only then -- if the device is that far behind --
// does push() wait for the block's readers.  Host-side only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "hip_host.hpp"

struct ListRing {
    static constexpr int kSlots = 4, kReaders = 2;      // readers: the caller's stream and the chain's tail stream
    HostMem<int32_t> host[kSlots];
    DevMem<int32_t> dev[kSlots];
    Event used[kSlots][kReaders];
    bool pending[kSlots][kReaders] = {};
    long long next = 0;

    // Copies list[0 .. n) into the next block and enqueues its upload on s.  capacity: the longest list this ring will ever carry
    // (the blocks are allocated once, at that size, on first use).  *d_list: the device copy, valid for kernels enqueued behind the
    // upload until done() has been told about their streams.  Returns the block's index (>= 0) or -1 with *err set.
    int push(const int32_t* list, int n, int capacity, hipStream_t s, int32_t** d_list, hipError_t* err) {
        const int k = (int)(next % kSlots);
        *err = hipSuccess;
        for (int r = 0; r < kReaders && *err == hipSuccess; r++)
            if (pending[k][r]) {
                *err = hipEventSynchronize(used[k][r]);
                pending[k][r] = false;
            }
        const size_t bytes = sizeof(int32_t) * (size_t)(capacity > 0 ? capacity : 1);
        if (*err == hipSuccess) *err = host[k].reserve(bytes);
        if (*err == hipSuccess) *err = dev[k].reserve(bytes);
        for (int r = 0; r < kReaders && *err == hipSuccess; r++)
            if (!used[k][r]) *err = hipEventCreateWithFlags(used[k][r].put(), hipEventDisableTiming);
        if (*err != hipSuccess) return -1;
        std::memcpy(host[k].get(), list, sizeof(int32_t) * (size_t)n);
        *err = hipMemcpyAsync(dev[k], host[k], sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s);
        if (*err != hipSuccess) return -1;
        next++;
        *d_list = dev[k];
        return k;
    }

    // Everything that reads block k on stream s (reader r) has been enqueued.
    hipError_t done(int k, int r, hipStream_t s) {
        const hipError_t e = hipEventRecord(used[k][r], s);
        if (e == hipSuccess) pending[k][r] = true;
        return e;
    }
};
