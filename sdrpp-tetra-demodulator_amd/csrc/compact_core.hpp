// compact_core.hpp -- "the rows that satisfy a predicate, in order": the one stream compaction of the receive chain, in three device
// functions.  A thread holds one row and a K-bit mask (bit k set <=> the row belongs to list k); a workgroup of ROWS threads holds
// ROWS consecutive rows.
//   block_count   per workgroup and list: its members -> work[k][block]
//   scan_counts   ONE workgroup: work[k][] -> exclusive prefix sums in place (the block's first position in list k), totals[k]
//   block_rank    per thread and list: members before it in its workgroup; position in list k = work[k][block] + rank
// Users: the compacting demultiplexer and the frame lists (tetra_burst_sync.hip), the CRC-good delivery (tetra_rx_out.hip).  Every
// hand-over between the three is a kernel boundary on one stream.
#pragma once

#include <hip/hip_runtime.h>

namespace compact_core {

// all threads of the workgroup call it (it holds barriers); row k of `work` is `stride` ints long
template <int K> __device__ __forceinline__ void block_count(unsigned mask, int* __restrict__ work, int stride, int block) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = __syncthreads_count((mask >> k) & 1u);
        if (threadIdx.x == 0) work[k * stride + block] = c;
    }
}

// One workgroup of FOUR wavefronts (a run of blocks per thread, shuffles within a wavefront, one exchange between the four): a
// workgroup has to find ONE compute unit with room for all its waves, and beside the demodulator -- whose 199-register waves leave
// 112 registers on two of a CU's four SIMDs -- a 1024-thread scan (four waves of 32 registers per SIMD) found none until the
// demodulator's launch was over: the tail of the receive chain then ran BEHIND the demodulator it was meant to overlap (two-stream
// chain 4.17 instead of 3.98 ms).
constexpr int kScanThreads = 256;
// all kScanThreads threads call it, once per kernel; row k holds len[k] >= 0 counts (a row of none gets total 0)
template <int K> __device__ __forceinline__ void scan_counts(int* __restrict__ work, int stride, const int (&len)[K], int* __restrict__ totals) {
    __shared__ int wave_sum[K][kScanThreads / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int lo[K], hi[K], sum[K], inc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int per = (len[k] + kScanThreads - 1) / kScanThreads;
        lo[k] = min(len[k], (int)threadIdx.x * per);
        hi[k] = min(len[k], lo[k] + per);
        sum[k] = 0;
        for (int i = lo[k]; i < hi[k]; ++i) sum[k] += work[k * stride + i];
        inc[k] = sum[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(inc[k], d);
            inc[k] += lane >= d ? v : 0;
        }
        if (lane == 63) wave_sum[k][w] = inc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int run = inc[k] - sum[k];
        for (int i = 0; i < w; ++i) run += wave_sum[k][i];
        for (int i = lo[k]; i < hi[k]; ++i) { const int c = work[k * stride + i]; work[k * stride + i] = run; run += c; }
        if (threadIdx.x == kScanThreads - 1) totals[k] = run;
    }
}

// all threads of the workgroup call it, once per kernel; the rows sit on its first ROWS threads (the others pass mask 0).
// total (may be null): the workgroup's members per list.
template <int K, int ROWS> __device__ __forceinline__ void block_rank(unsigned mask, int (&rank)[K], int* total = nullptr) {
    __shared__ int wave_cnt[K][ROWS / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned long long b = __ballot((mask >> k) & 1u);
        if (lane == 0 && w < ROWS / 64) wave_cnt[k][w] = __popcll(b);
        rank[k] = __popcll(b & ((1ull << lane) - 1ull));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int all = 0;
        for (int i = 0; i < ROWS / 64; ++i) {
            if (i < w) rank[k] += wave_cnt[k][i];
            all += wave_cnt[k][i];
        }
        if (total) total[k] = all;
    }
}

}  // namespace compact_core
