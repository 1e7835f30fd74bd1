// tetra_burst_scan.hip -- batched training-sequence search (include/tetra_burst_scan.h), bit-exact with the reference's
// tetra_find_train_seq() (src/decoder/src/phy/tetra_burst.c:271-341).
//
// One 256-thread workgroup per channel.  The row is walked in tiles of 32768 positions (scan_core::kTile): the tile's bytes
// (one bit each) are read once with coalesced 16-byte or dword loads and packed MSB-first into 32-bit words in LDS; every
// position then pulls its 22-bit look-ahead window out of two adjacent words with a funnel shift and compares it with the five
// sequence heads.  Candidates are verified against the full sequence (bytes, rare) and reduced with an LDS atomicMin on
// (position << 3 | check order), which is exactly "first position, then the reference's if-chain order".  The first 21
// positions reproduce the reference's misaligned pre-filter (see the header).  Integer/byte work: HBM-bound, every input
// byte is read from HBM once.  The code per word and per position is scan_core.hpp's, which tests/emul/scan_emul.cpp also
// builds for the host; this file keeps the loops, the barriers and the atomics.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../../include/tetra_burst_scan.h"
#include "hip_host.hpp"
#include "scan_core.hpp"

namespace {

using namespace scan_core;

static_assert(TETRA_TRAIN_NORM_1 == 0 && TETRA_TRAIN_NORM_2 == 1 && TETRA_TRAIN_NORM_3 == 2 && TETRA_TRAIN_SYNC == 3 && TETRA_TRAIN_EXT == 4,
              "scan_core::c_type holds these values as numbers");

__global__ __launch_bounds__(kThreads) void k_find_train_seq(const uint8_t* bits, int bits_stride, const int* end_of_in,
                                                             unsigned mask, int* type_out, int* off_out) {
    __shared__ unsigned packed[kTileWords];
    __shared__ unsigned best;              // (cur << 3) | check-order index
    __shared__ unsigned heads[5];
    const int ch = blockIdx.x;
    const uint8_t* in = bits + (long long)ch * bits_stride;
    const int end = clamp_end(end_of_in[ch], bits_stride);
    if (threadIdx.x == 0) best = kNone;
    if (threadIdx.x < 5) heads[threadIdx.x] = head22(threadIdx.x);
    __syncthreads();

    if (threadIdx.x == 0 && end > 0) {
        unsigned filter = 0;                                             // (the seed as a function of scan_core.hpp makes the compiler
        for (int i = 0; i < 20; i++) filter = (filter << 1) | in[i];     // split this 20-byte load in five: kept here, profiles/HISTORY.md)
        const int lim = end < kEarly ? end : kEarly;
        for (int cur = 0; cur < lim; cur++) {
            filter = prefilter_step(filter, in, cur);
            bool m = false;
            for (int s = 0; s < 5; s++) m |= (filter == heads[s]);
            if (m) {
                const int s = verify(in, cur, end, mask);
                if (s < 5) { atomicMin(&best, match_key(cur, s)); break; }
            }
        }
    }

    for (int base = 0; base < end; base += kTile) {
        __syncthreads();
        if (scan_done(best, base)) break;                                // (uniform)
        // pack bytes [base, base + kTile + 64) to bits
        for (int w = threadIdx.x; w < kTileWords; w += kThreads) packed[w] = pack_word(in, base + 32 * w, bits_stride);
        __syncthreads();
        const int lim = (end - base < kTile) ? (end - base) : kTile;
        for (int r = threadIdx.x; r < lim; r += kThreads) {
            if (candidate(packed, heads, base, r)) {
                const int s = verify(in, base + r, end, mask);
                if (s < 5) atomicMin(&best, match_key(base + r, s));
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (best == kNone) { type_out[ch] = -1; off_out[ch] = -1; }
        else { type_out[ch] = c_type[best & 7u]; off_out[ch] = (int)(best >> 3); }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The plugin's indicator (src/main.cpp:385-414): see tetra_burst_scan.h.  One 256-thread workgroup per channel; the stream
// v = [carried 44 bits | this call's bits] is packed MSB-first into LDS tile by tile like above, every position pulls its
// 45-bit window out of three adjacent words and compares its head with the eight sequences; the last hit is an LDS atomicMax.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_ts_indicator(const uint8_t* bits, int bits_stride, const int* n_bits, uint8_t* tail,
                                                           int* expire, uint8_t* found_out, int* expire_out) {
    __shared__ unsigned packed[kIndTileWords];
    __shared__ unsigned long long heads[8];       // sequence s as the top c_ind_len[s] bits of a 45-bit window
    __shared__ uint8_t new_tail[kIndTail];
    __shared__ int last_hit;
    const int ch = blockIdx.x;
    const uint8_t* in = bits + (long long)ch * bits_stride;
    uint8_t* tl = tail + (long long)ch * kIndTail;
    const int n = ind_clamp(n_bits[ch], bits_stride);
    if (threadIdx.x == 0) last_hit = -1;
    if (threadIdx.x < 8) heads[threadIdx.x] = ind_head(threadIdx.x);
    for (int base = 0; base < n; base += kIndTile) {
        __syncthreads();
        for (int w = threadIdx.x; w < kIndTileWords; w += kThreads) packed[w] = ind_pack_word(tl, in, n, base + 32 * w);
        __syncthreads();
        const int lim = (n - base < kIndTile) ? (n - base) : kIndTile;
        int mine = -1;
        for (int r = threadIdx.x; r < lim; r += kThreads)
            if (ind_hit(packed, heads, r)) mine = base + r;       // r ascends: the thread's last hit
        if (mine >= 0) atomicMax(&last_hit, mine);
    }
    __syncthreads();
    if (n > 0) {
        if (threadIdx.x < kIndTail) new_tail[threadIdx.x] = (uint8_t)ind_vbit(tl, in, n, n + threadIdx.x);
        __syncthreads();
        if (threadIdx.x < kIndTail) tl[threadIdx.x] = new_tail[threadIdx.x];
    }
    if (threadIdx.x == 0) {
        int e = expire[ch];
        if (n > 0) {
            e = ind_expire(e, n, last_hit);
            expire[ch] = e;
        }
        found_out[ch] = e > 0 ? 1 : 0;
        if (expire_out) expire_out[ch] = e;
    }
}

}  // namespace

extern "C" {

int tetra_find_train_seq_batch_device(const uint8_t* d_bits, int n_channels, int bits_stride, const int32_t* d_end_of_in,
                                      uint32_t mask, int32_t* d_type, int32_t* d_offset, void* hip_stream) {
    if (!d_bits || !d_end_of_in || !d_type || !d_offset || n_channels < 1 || bits_stride < 4) return TETRA_ERR_ARG;
    if ((bits_stride & 3) || (reinterpret_cast<uintptr_t>(d_bits) & 3)) return TETRA_ERR_ALIGN;
    hipLaunchKernelGGL(k_find_train_seq, dim3(n_channels), dim3(kThreads), 0, (hipStream_t)hip_stream, d_bits, bits_stride,
                       d_end_of_in, mask, d_type, d_offset);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_find_train_seq_batch(const uint8_t* bits, int n_channels, int bits_stride, const int32_t* end_of_in, uint32_t mask,
                               int32_t* type, int32_t* offset, int device) {
    if (!bits || !end_of_in || !type || !offset || n_channels < 1 || bits_stride < 4) return TETRA_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    if (device >= ndev) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    DevMem<uint8_t> d_bits;
    DevMem<int> d_end, d_t, d_o;
    const size_t nb = (size_t)n_channels * (size_t)bits_stride;
    if (d_bits.reserve(nb) != hipSuccess || d_end.reserve(sizeof(int) * n_channels) != hipSuccess ||
        d_t.reserve(sizeof(int) * n_channels) != hipSuccess || d_o.reserve(sizeof(int) * n_channels) != hipSuccess)
        return TETRA_ERR_NOMEM;
    if (hipMemcpy(d_bits, bits, nb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_end, end_of_in, sizeof(int) * n_channels, hipMemcpyHostToDevice) != hipSuccess)
        return TETRA_ERR_HIP;
    const int rc = tetra_find_train_seq_batch_device(d_bits, n_channels, bits_stride, d_end, mask, d_t, d_o, nullptr);
    if (rc != TETRA_OK) return rc;
    if (hipStreamSynchronize(0) != hipSuccess || hipMemcpy(type, d_t, sizeof(int) * n_channels, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(offset, d_o, sizeof(int) * n_channels, hipMemcpyDeviceToHost) != hipSuccess)
        return TETRA_ERR_HIP;
    return TETRA_OK;
}

struct tetra_ts_indicator {
    int C = 0, device = 0;
    DevMem<uint8_t> tail;         // [C][44]
    DevMem<int> expire;           // [C]
};

int tetra_ts_indicator_create(int n_channels, int device, tetra_ts_indicator_t** out) {
    if (!out) return TETRA_ERR_ARG;
    *out = nullptr;
    if (n_channels < 1) return TETRA_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return TETRA_ERR_NO_DEVICE;
    if (device >= ndev) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    tetra_ts_indicator* h = new (std::nothrow) tetra_ts_indicator;
    if (!h) return TETRA_ERR_NOMEM;
    h->C = n_channels;
    h->device = device;
    if (h->tail.reserve((size_t)n_channels * kIndTail) != hipSuccess || h->expire.reserve(sizeof(int) * (size_t)n_channels) != hipSuccess) {
        delete h;
        return TETRA_ERR_NOMEM;
    }
    const int rc = tetra_ts_indicator_reset(h, -1);
    if (rc != TETRA_OK) { delete h; return rc; }
    *out = h;
    return TETRA_OK;
}

void tetra_ts_indicator_destroy(tetra_ts_indicator_t* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    delete h;
}

int tetra_ts_indicator_reset(tetra_ts_indicator_t* h, int channel) {
    if (!h || channel < -1 || channel >= h->C) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    const size_t first = channel < 0 ? 0 : (size_t)channel, count = channel < 0 ? (size_t)h->C : 1;
    if (hipMemset(h->tail + first * kIndTail, 0, count * kIndTail) != hipSuccess ||
        hipMemset(h->expire + first, 0, sizeof(int) * count) != hipSuccess)
        return TETRA_ERR_HIP;
    return TETRA_OK;
}

int tetra_ts_indicator_process_device(tetra_ts_indicator_t* h, const uint8_t* d_bits, int bits_stride, const int32_t* d_n_bits,
                                      uint8_t* d_found, int32_t* d_expire, void* hip_stream) {
    if (!h || !d_bits || !d_n_bits || !d_found || bits_stride < 4) return TETRA_ERR_ARG;
    if ((bits_stride & 3) || (reinterpret_cast<uintptr_t>(d_bits) & 3)) return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipLaunchKernelGGL(k_ts_indicator, dim3(h->C), dim3(kThreads), 0, (hipStream_t)hip_stream, d_bits, bits_stride, d_n_bits,
                       h->tail, h->expire, d_found, d_expire);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_ts_indicator_process(tetra_ts_indicator_t* h, const uint8_t* bits, int bits_stride, const int32_t* n_bits,
                               uint8_t* found, int32_t* expire) {
    if (!h || !bits || !n_bits || !found || bits_stride < 4) return TETRA_ERR_ARG;
    if (bits_stride & 3) return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    DevMem<uint8_t> d_bits, d_found;
    DevMem<int> d_n, d_e;
    const size_t nb = (size_t)h->C * (size_t)bits_stride;
    if (d_bits.reserve(nb) != hipSuccess || d_n.reserve(sizeof(int) * h->C) != hipSuccess || d_found.reserve((size_t)h->C) != hipSuccess ||
        d_e.reserve(sizeof(int) * h->C) != hipSuccess)
        return TETRA_ERR_NOMEM;
    if (hipMemcpy(d_bits, bits, nb, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_n, n_bits, sizeof(int) * h->C, hipMemcpyHostToDevice) != hipSuccess)
        return TETRA_ERR_HIP;
    const int rc = tetra_ts_indicator_process_device(h, d_bits, bits_stride, d_n, d_found, d_e, nullptr);
    if (rc != TETRA_OK) return rc;
    if (hipStreamSynchronize(0) != hipSuccess || hipMemcpy(found, d_found, (size_t)h->C, hipMemcpyDeviceToHost) != hipSuccess ||
        (expire && hipMemcpy(expire, d_e, sizeof(int) * h->C, hipMemcpyDeviceToHost) != hipSuccess))
        return TETRA_ERR_HIP;
    return TETRA_OK;
}

}  // extern "C"
