// tetra_iqcond.hip -- the handle-free entry points of the capture conditioning (include/ext/tetra_iqcond.h): the statistics of a capture
// on the device, in one pass, and the solver that turns them into an input map (host only).  The map itself is applied inside the
// channeliser's loads (tetra_chan.hip, chan_fft_core.hpp); the lane code of both is iqcond_core.hpp.
//
// Statistics, two stages (the pattern of tetra_wbrx.hip's bin power):
//   k_iq_stats_part   grid-stride over the samples, five sums per lane, a fixed tree over the workgroup in LDS, one row of five per
//                     workgroup into scratch -- plain vector stores, no atomics
//   k_iq_stats_sum    one workgroup: the rows in a fixed order per lane, the same tree, five values out
// Integer formats accumulate in int64 (exact: the result does not depend on any order); complex64 in double, in an order that the
// grid fixes -- and the grid is a function of n alone, not of the device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/ext/tetra_iqcond.h"
#include "chan_fft_core.hpp"
#include "hip_host.hpp"
#include "iqcond_core.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 16;          // samples per lane before a call gets another workgroup ...
constexpr int kMaxGroups = 2048;      // ... up to this many (then the lanes loop on): 8 per CU of work in flight on 256 CUs

// the workgroup's tree over s[kThreads] (LDS), result in s[0]: the same pairing whatever the data
template <class T> __device__ __forceinline__ void reduce_block(iqcond::Sums<T>* s, int tid) {
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) iqcond::add_sums(s[tid], s[tid + off]);
        __syncthreads();
    }
}

// FMT: chanfft::kFmtC32 / kFmtCs16 / kFmtCs8.  part: [gridDim.x] rows of five
template <int FMT, class T> __global__ __launch_bounds__(kThreads) void k_iq_stats_part(const void* __restrict__ x, long long n, iqcond::Sums<T>* __restrict__ part) {
    __shared__ iqcond::Sums<T> s[kThreads];
    const int tid = threadIdx.x;
    iqcond::Sums<T> acc = {};
    const long long stride = (long long)gridDim.x * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + tid; i < n; i += stride) {
        if constexpr (FMT == chanfft::kFmtCs16) {
            const chanfft::cs16 v = reinterpret_cast<const chanfft::cs16*>(x)[i];
            iqcond::add_sample(acc, v.x, v.y);
        } else if constexpr (FMT == chanfft::kFmtCs8) {
            const chanfft::cs8 v = reinterpret_cast<const chanfft::cs8*>(x)[i];
            iqcond::add_sample(acc, v.x, v.y);
        } else {
            const chanfft::c32 v = reinterpret_cast<const chanfft::c32*>(x)[i];
            iqcond::add_sample(acc, v.x, v.y);
        }
    }
    s[tid] = acc;
    reduce_block(s, tid);
    if (tid == 0) part[blockIdx.x] = s[0];
}

template <class T> __global__ __launch_bounds__(kThreads) void k_iq_stats_sum(const iqcond::Sums<T>* __restrict__ part, int rows, iqcond::Sums<T>* __restrict__ out) {
    __shared__ iqcond::Sums<T> s[kThreads];
    const int tid = threadIdx.x;
    iqcond::Sums<T> acc = {};
    for (int j = tid; j < rows; j += kThreads) iqcond::add_sums(acc, part[j]);
    s[tid] = acc;
    reduce_block(s, tid);
    if (tid == 0) out[0] = s[0];
}

constexpr int kFmtBytes[3] = { 8, 4, 2 };

// scratch [groups + 1] rows: the partial rows, then the result
template <int FMT, class T> hipError_t run(const void* d_x, long long n, int groups, void* scratch, T host[iqcond::kSums], hipStream_t s) {
    iqcond::Sums<T>* part = static_cast<iqcond::Sums<T>*>(scratch);
    hipLaunchKernelGGL((k_iq_stats_part<FMT, T>), dim3((unsigned)groups), dim3(kThreads), 0, s, d_x, n, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_iq_stats_sum<T>), dim3(1), dim3(kThreads), 0, s, part, groups, part + groups);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(host, part + groups, sizeof(T) * iqcond::kSums, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

}  // namespace

extern "C" {

int tetra_iq_stats_device(const void* d_x, int fmt, long long n, tetra_iq_stats_t* out, void* hip_stream) {
    if (!out || fmt < 0 || fmt > 2 || (!d_x && n > 0)) return TETRA_ERR_ARG;
    if (n < 0 || (fmt != chanfft::kFmtC32 && n > (1LL << 32))) return TETRA_ERR_SIZE;
    if ((uintptr_t)d_x & (uintptr_t)(kFmtBytes[fmt] - 1)) return TETRA_ERR_ALIGN;
    std::memset(out, 0, sizeof(*out));
    if (n == 0) return TETRA_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // the grid from n alone (not from the device): it fixes the order of the complex64 sums
    const long long want = (n + (long long)kThreads * kPerLane - 1) / ((long long)kThreads * kPerLane);
    const int groups = (int)(want < kMaxGroups ? want : kMaxGroups);
    DevMem<unsigned char> scratch;
    if (scratch.reserve(sizeof(iqcond::Sums<double>) * ((size_t)groups + 1)) != hipSuccess) return TETRA_ERR_NOMEM;
    hipError_t e;
    if (fmt == chanfft::kFmtC32) {
        double v[iqcond::kSums];
        e = run<chanfft::kFmtC32, double>(d_x, n, groups, scratch.get(), v, s);
        if (e != hipSuccess) return TETRA_ERR_HIP;
        out->s_i = v[0]; out->s_q = v[1]; out->s_ii = v[2]; out->s_qq = v[3]; out->s_iq = v[4];
    } else {
        long long v[iqcond::kSums];
        e = fmt == chanfft::kFmtCs16 ? run<chanfft::kFmtCs16, long long>(d_x, n, groups, scratch.get(), v, s)
                                     : run<chanfft::kFmtCs8, long long>(d_x, n, groups, scratch.get(), v, s);
        if (e != hipSuccess) return TETRA_ERR_HIP;
        // (double) of an int64 rounds correctly (to nearest even); the power-of-two scale is exact
        const int sh = fmt == chanfft::kFmtCs16 ? 15 : 7;
        out->s_i = std::ldexp((double)v[0], -sh);
        out->s_q = std::ldexp((double)v[1], -sh);
        out->s_ii = std::ldexp((double)v[2], -2 * sh);
        out->s_qq = std::ldexp((double)v[3], -2 * sh);
        out->s_iq = std::ldexp((double)v[4], -2 * sh);
    }
    out->n = n;
    return TETRA_OK;
}

int tetra_iq_map_from_stats(const tetra_iq_stats_t* st, tetra_iq_map_t* map) {
    if (!st || !map || st->n < 2) return TETRA_ERR_ARG;
    // in double, operation by operation as the header states it (this file is compiled without contraction)
    const double n = (double)st->n;
    const double uI = st->s_i / n, uQ = st->s_q / n;
    const double A = st->s_ii / n - uI * uI;
    const double B = st->s_qq / n - uQ * uQ;
    const double C = st->s_iq / n - uI * uQ;
    if (!(A > 0)) return TETRA_ERR_ARG;
    const double den = B - C * C / A;
    if (!(den > 0)) return TETRA_ERR_ARG;
    const double r = C / A;
    const double k = std::sqrt(A / den);
    const iqcond::Map m = { 1.f, 0.f, (float)(-(k * r)), (float)k, (float)(-uI), (float)(k * (r * uI - uQ)) };
    if (!iqcond::finite(m)) return TETRA_ERR_ARG;
    map->m00 = m.m00; map->m01 = m.m01; map->m10 = m.m10; map->m11 = m.m11; map->c0 = m.c0; map->c1 = m.c1;
    return TETRA_OK;
}

}  // extern "C"
