// tetra_burst_sync.hip -- batched burst synchroniser + burst demultiplexer (include/tetra_burst_sync.h).
//
// k_burst_sync / k_burst_sync_tol (the reference's lock rule / the tolerant one, include/ext/tetra_sync_tol.h; one body,
// burst_sync_workgroup, with the rule as a parameter): one workgroup of four wavefronts per channel (the byte work of steps 1, 2 and 4
// on all 256 lanes; step 3 on one wave).
//   1. the channel's stream of this call -- carried buffer (<= 4096 bits, one byte per bit in HBM) followed by the new
//      bits -- is packed 32 bits per word into LDS; the new bits start word-aligned, 32 bytes -> one word per lane-step
//      with 16-byte loads and one multiply per 8 bytes (the scan kernel's trick);
//   2. the rule's match bitmaps (sync / normal 1 / normal 2 training sequence present at x and their union, or sync alone) are built
//      32 positions per lane-step;
//   3. the wave walks the event-driven state machine of bsync_core.hpp (about 70 events per second of signal) in lock
//      step; its "first set bit in [a, b)" searches over the bitmaps are wave-cooperative (one word per lane + ballot);
//      the consumed frames are listed in LDS;
//   4. all lanes expand the listed frames to one byte per bit with coalesced dword stores, and write the new carried
//      buffer and the state.
// Steps 1 and 4 and the walk are lane code in bsync_core.hpp, which the host emulation runs too.
// Byte work: every input byte is read from HBM once, every output byte written once.
// k_burst_sync_assist / k_burst_sync_tol_assist: the same body with the hand-over's state ASSIST beside the rule (bsync_core.hpp:
// AssistLock; include/ext/tetra_handover.h), launched instead of the two above once a handle has handed over.
// k_burst_demux: one thread per output dword; a gather with the offsets of tetra_burst_rx_cb().
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/ext/tetra_sync_tol.h"
#include "../../include/tetra_burst_sync.h"
#include "bsync_core.hpp"
#include "compact_core.hpp"
#include "demux_core.hpp"
#include "hip_host.hpp"
#include "retune_impl.hpp"

namespace {

using namespace bsync_core;

constexpr int kLanes = 64;
constexpr int kThreadsBS = kThreads;  // k_burst_sync: four wavefronts per channel for the byte work, one of them walks the state machine
constexpr int kMaxBitsLimit = 262144;
static_assert(kFrameWords == TETRA_FRAME_WORDS && kFrameStride == TETRA_FRAME_STRIDE, "frame layout");

// walk()'s `first` for a wavefront in lock step: one word per lane + ballot
__device__ __forceinline__ int first_wave(const uint32_t* m, int a, int b, int lane) {
    if (a >= b) return -1;
    const int w0 = a >> 5, w1 = (b - 1) >> 5;
    for (int base = w0; base <= w1; base += kLanes) {
        const int w = base + lane;
        uint32_t v = (w <= w1) ? m[w] : 0u;
        if (w == w0) v &= 0xffffffffu << (a & 31);
        if (w == w1 && (b & 31) != 0) v &= (1u << (b & 31)) - 1u;
        const unsigned long long hit = __ballot(v != 0u);
        if (hit) {
            const int l = __builtin_ctzll(hit);
            return 32 * (base + l) + __builtin_ctz(__shfl(v, l));
        }
    }
    return -1;
}

// What a lock rule says to the workgroup: how many bitmaps lie behind the stream in LDS (m [kMaps][words], the sync bitmap first) and
// how word w of them is built; where the channel's rule state is loaded and stored and its policy object for walk(); and one
// round of the LOCKED batch -- the lane's frame [bx, bx + 510) evaluated if `active` (lanes 0 .. here - 1), -> what it reports, and
// the index of the lane behind whose frame the receiver unlocks, or -1.
struct RefRule {          // the reference's rule: sync / normal 1 / normal 2 bitmaps and their union
    static constexpr int kMaps = 4;
    __device__ void map_word(const uint32_t* s, uint32_t* m, int words, int w, bool inside, int x0, int xe) const {
        uint32_t a = 0, b = 0, c = 0;
        if (inside) match_word(s, w, x0, xe, a, b, c);
        m[w] = a;
        m[words + w] = b;
        m[2 * words + w] = c;
        m[3 * words + w] = a | b | c;
    }
    __device__ int load(int) const { return 0; }
    __device__ void store(int, int) const {}
    __device__ RefLock lock(const uint32_t* m, int words, int&) const { return RefLock{ m, m + words, m + 2 * words, m + 3 * words }; }
    __device__ int round(RefLock& lock, const uint32_t* s, int bx, bool active, int, int& reported) const {
        FrameEval e = { -1, false };
        if (active) e = locked_frame_eval(s, lock.m_sync, lock.m_n1, lock.m_n2, lock.m_any, bx);
        reported = e.reported;
        const unsigned long long um = __ballot(e.unlocks);
        return um ? __builtin_ctzll(um) : -1;
    }
};
// The tolerant lock (include/ext/tetra_sync_tol.h): the sync bitmap only; a lane evaluates the three windows of its frame
// (tolerant_frame_eval) and the consecutive-miss rule runs over the ballot of the reported frames (first_unlock_bits).  miss [C]: the
// channels' miss counters beside their State.
struct TolRule {
    static constexpr int kMaps = 1;
    Tolerance tol;
    int32_t* miss;
    __device__ void map_word(const uint32_t* s, uint32_t* m, int, int w, bool inside, int x0, int xe) const {
        m[w] = inside ? match_word_sync(s, w, x0, xe) : 0u;
    }
    __device__ int load(int ch) const { return miss[ch]; }
    __device__ void store(int ch, int misses) const { miss[ch] = misses; }
    __device__ TolLock lock(const uint32_t*, int, int& misses) const { return TolLock{ tol, misses }; }
    __device__ int round(TolLock& lock, const uint32_t* s, int bx, bool active, int here, int& reported) const {
        reported = active ? tolerant_frame_eval(s, bx, lock.tol) : -1;
        const Unlock u = first_unlock_bits(__ballot(reported >= 0), here, lock.misses, lock.tol.max_miss);
        lock.misses = u.misses;
        return u.index;
    }
};

// One workgroup of four wavefronts per channel (steps 1 .. 4 of the head of this file).
// PACKED: the consumed frames leave as 16 words of 32 bits (first bit = most significant; word 15 holds bits 480 .. 509 in its top 30
// bits) instead of 512 bytes: an eighth of the bytes for the demultiplexer behind (tetra_bsync_process_packed_device).
// ASSIST: the hand-over's state beside the rule's (include/ext/tetra_handover.h): the channel's Assist is loaded, walk() runs under
// AssistLock around the rule's policy, and lane 0 stores it back.  The kernels of a handle that never handed over are compiled without.
template <bool PACKED, class Rule, bool ASSIST = false>
__device__ __forceinline__ void burst_sync_workgroup(const Rule rule, const uint8_t* __restrict__ bits, int bits_stride, const int* __restrict__ n_bits,
                                                     int max_bits, int max_frames, State* __restrict__ states, uint8_t* __restrict__ carry,
                                                     uint8_t* __restrict__ frames, int* __restrict__ frame_type,
                                                     uint32_t* __restrict__ frame_bitnum, int* __restrict__ n_frames, Assist* __restrict__ assist = nullptr) {
    extern __shared__ uint32_t lds[];
    const int words = stream_words(max_bits);
    uint32_t* s = lds;
    uint32_t* maps = s + words;
    FrameRec* rec = reinterpret_cast<FrameRec*>(maps + Rule::kMaps * words);
    __shared__ int sh_nframes, sh_carry_x;
    __shared__ State sh_state;

    const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & (kLanes - 1);
    uint8_t* cbuf = carry + (size_t)ch * kBuf;
    State st = states[ch];
    int n_new = n_bits[ch];
    n_new = n_new < 0 ? 0 : (n_new > max_bits ? max_bits : n_new);
    n_new = n_new > bits_stride ? bits_stride : n_new;         // a poisoned count never reads into the next channel's row
    const int x0 = kOff - (int)st.bits_in_buf, xe = kOff + n_new;

    // 1. pack the stream
    stage_thread(tid, s, words, x0, n_new, cbuf, bits + (size_t)ch * bits_stride);
    __syncthreads();

    // 2. match bitmaps
    for (int w = tid; w < words; w += kThreadsBS) rule.map_word(s, maps, words, w, w + 2 < words && 32 * w + 32 > x0 && 32 * w < xe, x0, xe);
    __syncthreads();

    // 3. state machine: all lanes in lock step (uniform control flow); the bitmap searches are wave-cooperative
    if (tid < kLanes) {      // (one wavefront walks the events; the other three join again for the byte work behind the barrier)
        int carry_x = 0;
        int rule_state = rule.load(ch);
        auto lock = rule.lock(maps, words, rule_state);
        // LOCKED steady state: one frame per lane, 64 per round, up to and including the first frame that unlocks the receiver
        auto batch = [&](int bx, int K, int f0, uint32_t abs_bx, bool& unlocked) -> int {
            int done = 0;
            while (done < K) {
                const int k = done + lane, here = K - done < kLanes ? K - done : kLanes;
                int reported;
                const int stop = rule.round(lock, s, bx + kTs * k, lane < here, here, reported);
                const int take = stop >= 0 ? stop + 1 : here;
                if (lane < take && f0 + k < max_frames) rec[f0 + k] = FrameRec{ bx + kTs * k, reported, abs_bx + (uint32_t)(kTs * k) };
                done += take;
                if (stop >= 0) { unlocked = true; break; }
            }
            return done;
        };
        auto first = [&](const uint32_t* m, int a, int b) { return first_wave(m, a, b, lane); };
        auto emit = [&](int f, int bx, int type, uint32_t bitnum) {
            if (lane == 0 && f < max_frames) rec[f] = FrameRec{ bx, type, bitnum };
        };
        int nrun;
        if constexpr (ASSIST) {
            Assist as = assist[ch];
            AssistLock<decltype(lock)> with_assist{ lock, as };
            nrun = walk(st, s, maps, n_new, carry_x, first, emit, batch, with_assist);
            if (lane == 0) assist[ch] = as;
        } else {
            nrun = walk(st, s, maps, n_new, carry_x, first, emit, batch, lock);
        }
        if (lane == 0) {
            rule.store(ch, rule_state);
            sh_nframes = nrun < max_frames ? nrun : max_frames;
            sh_carry_x = carry_x;
            sh_state = st;
        }
    }
    __syncthreads();

    // 4. frames, carry, state
    const int nf = sh_nframes;
    write_thread<PACKED>(tid, s, rec, nf, max_frames, TETRA_FRAME_NONE, sh_carry_x, xe,
                         frames + (size_t)ch * max_frames * (PACKED ? TETRA_FRAME_WORDS * 4 : TETRA_FRAME_STRIDE),
                         frame_type + (size_t)ch * max_frames, frame_bitnum + (size_t)ch * max_frames, cbuf);
    if (tid == 0) {
        states[ch] = sh_state;
        n_frames[ch] = nf;
    }
}

template <bool PACKED> __global__ __launch_bounds__(kThreadsBS) void k_burst_sync(const uint8_t* __restrict__ bits, int bits_stride, const int* __restrict__ n_bits,
                                                       int max_bits, int max_frames, State* __restrict__ states,
                                                       uint8_t* __restrict__ carry, uint8_t* __restrict__ frames,
                                                       int* __restrict__ frame_type, uint32_t* __restrict__ frame_bitnum,
                                                       int* __restrict__ n_frames) {
    burst_sync_workgroup<PACKED>(RefRule{}, bits, bits_stride, n_bits, max_bits, max_frames, states, carry, frames, frame_type, frame_bitnum, n_frames);
}
template <bool PACKED> __global__ __launch_bounds__(kThreadsBS) void k_burst_sync_tol(const uint8_t* __restrict__ bits, int bits_stride, const int* __restrict__ n_bits,
                                                       int max_bits, int max_frames, State* __restrict__ states,
                                                       uint8_t* __restrict__ carry, uint8_t* __restrict__ frames,
                                                       int* __restrict__ frame_type, uint32_t* __restrict__ frame_bitnum,
                                                       int* __restrict__ n_frames, const Tolerance tol, int32_t* __restrict__ miss) {
    burst_sync_workgroup<PACKED>(TolRule{ tol, miss }, bits, bits_stride, n_bits, max_bits, max_frames, states, carry, frames, frame_type, frame_bitnum, n_frames);
}

// ... and the same two for a handle that has handed over (include/ext/tetra_handover.h): assist [C] beside the states
template <bool PACKED> __global__ __launch_bounds__(kThreadsBS) void k_burst_sync_assist(const uint8_t* __restrict__ bits, int bits_stride, const int* __restrict__ n_bits,
                                                       int max_bits, int max_frames, State* __restrict__ states,
                                                       uint8_t* __restrict__ carry, uint8_t* __restrict__ frames,
                                                       int* __restrict__ frame_type, uint32_t* __restrict__ frame_bitnum,
                                                       int* __restrict__ n_frames, Assist* __restrict__ assist) {
    burst_sync_workgroup<PACKED, RefRule, true>(RefRule{}, bits, bits_stride, n_bits, max_bits, max_frames, states, carry, frames, frame_type, frame_bitnum, n_frames, assist);
}
template <bool PACKED> __global__ __launch_bounds__(kThreadsBS) void k_burst_sync_tol_assist(const uint8_t* __restrict__ bits, int bits_stride, const int* __restrict__ n_bits,
                                                       int max_bits, int max_frames, State* __restrict__ states,
                                                       uint8_t* __restrict__ carry, uint8_t* __restrict__ frames,
                                                       int* __restrict__ frame_type, uint32_t* __restrict__ frame_bitnum,
                                                       int* __restrict__ n_frames, const Tolerance tol, int32_t* __restrict__ miss, Assist* __restrict__ assist) {
    burst_sync_workgroup<PACKED, TolRule, true>(TolRule{ tol, miss }, bits, bits_stride, n_bits, max_bits, max_frames, states, carry, frames, frame_type, frame_bitnum, n_frames, assist);
}

using demux_core::Pieces;
using demux_core::PiecesLut;
using demux_core::pieces_for;
using demux_core::lut_for;

// The demultiplexer kernels: thread-level code in demux_core.hpp (shared with the host emulation).
// one thread per output dword -- or, WIDE (rows a multiple of 8 bytes, 8-byte aligned), per pair of dwords: half the threads, 8-byte stores
template <bool PACKED, bool WIDE> __global__ __launch_bounds__(256) void k_burst_demux(const uint8_t* __restrict__ frames, const int* __restrict__ frame_type, int n,
                                                     int tpsap, int blk_num, uint8_t* __restrict__ rows, int row_stride,
                                                     int* __restrict__ valid) {
    demux_core::demux_thread<PACKED, WIDE>(blockIdx.x, threadIdx.x, frames, frame_type, n, tpsap, blk_num, rows, row_stride, valid);
}

// ---- compaction (compact_core.hpp): list k of a call = the frames r whose mask(r) has bit k set, in frame order ----
// The compacting form of the demultiplexer is K = 1 (CarriesKind: only frames that carry the block kind produce a row), the frame
// lists of tetra_burst_index_device K = TETRA_N_LISTS (ListMask).
constexpr int kRows = 256;            // frames per workgroup of k_list_count / k_list_write
// 1. entries per kRows frames and list
template <int K, class Mask> __global__ __launch_bounds__(kRows) void k_list_count(const Mask mask, int n, int nblocks, int* __restrict__ work) {
    const int r = blockIdx.x * kRows + threadIdx.x;
    compact_core::block_count<K>(r < n ? mask(r) : 0u, work, nblocks, blockIdx.x);
}
// 2. exclusive scan of each list's block counts, totals -> counts
template <int K> __global__ __launch_bounds__(compact_core::kScanThreads) void k_list_scan(int* __restrict__ work, int nblocks, int* __restrict__ counts) {
    int len[K];
#pragma unroll
    for (int k = 0; k < K; ++k) len[k] = nblocks;
    compact_core::scan_counts<K>(work, nblocks, len, counts);
}
// 3. the lists themselves [K][n], and (the frame lists only: chan_first != null) per channel the position of its first entry
template <int K, class Mask> __global__ __launch_bounds__(kRows) void k_list_write(const Mask mask, int n, int nblocks, int frames_per_channel,
                                                                                  const int* __restrict__ work, int* __restrict__ lists, int* __restrict__ chan_first) {
    const int r = blockIdx.x * kRows + threadIdx.x;
    const unsigned m = r < n ? mask(r) : 0u;
    int at[K];
    compact_core::block_rank<K, kRows>(m, at);
    const bool first_of_channel = chan_first && r < n && r % frames_per_channel == 0;
    const int chans = first_of_channel ? n / frames_per_channel : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        at[k] += work[k * nblocks + blockIdx.x];
        if ((m >> k) & 1u) lists[(size_t)k * n + at[k]] = r;
        if (first_of_channel) chan_first[(size_t)k * chans + r / frames_per_channel] = at[k];
    }
}
template <int K, class Mask> void lists_launch(const Mask& mask, int n, int frames_per_channel, int* work, int* lists, int* counts, int* chan_first, hipStream_t s) {
    const int nblocks = (n + kRows - 1) / kRows;
    hipLaunchKernelGGL((k_list_count<K, Mask>), dim3(nblocks), dim3(kRows), 0, s, mask, n, nblocks, work);
    hipLaunchKernelGGL(k_list_scan<K>, dim3(1), dim3(compact_core::kScanThreads), 0, s, work, nblocks, counts);
    hipLaunchKernelGGL((k_list_write<K, Mask>), dim3(nblocks), dim3(kRows), 0, s, mask, n, nblocks, frames_per_channel, work, lists, chan_first);
}
struct CarriesKind {      // the compacting demultiplexer's one list
    const int* frame_type; int tpsap, blk_num;
    __device__ unsigned operator()(int r) const { return pieces_for(frame_type[r], tpsap, blk_num).len0 > 0; }
};
struct ListMask {         // the frame lists of a call (tetra_burst_index_device): SYNC / NORM_1 / NORM_2 / any
    const int* frame_type;
    __device__ unsigned operator()(int r) const {
        const int t = frame_type[r];
        return t == TETRA_TRAIN_SYNC ? (1u << TETRA_LIST_SYNC) | (1u << TETRA_LIST_ANY)
             : t == TETRA_TRAIN_NORM_1 ? (1u << TETRA_LIST_NORM_1) | (1u << TETRA_LIST_ANY)
             : t == TETRA_TRAIN_NORM_2 ? (1u << TETRA_LIST_NORM_2) | (1u << TETRA_LIST_ANY) : 0u;
    }
};

// the gather itself, one thread per output dword of the worst case; rows past *n_rows do not exist
template <bool PACKED, bool WIDE> __global__ __launch_bounds__(256) void k_demux_gather(const uint8_t* __restrict__ frames, const int* __restrict__ frame_type,
                                                      const int* __restrict__ row_frame, const int* __restrict__ n_rows, int n,
                                                      int tpsap, int blk_num, uint8_t* __restrict__ rows, int row_stride) {
    demux_core::gather_thread<PACKED, WIDE>(blockIdx.x, threadIdx.x, frames, frame_type, row_frame, *n_rows, n, tpsap, blk_num, rows, row_stride);
}

// PACKED frames, 8-byte row units, rows of at most 512 bytes: whole rows per wavefront (demux_core::rows_thread).  GATHER: the compacted rows.
template <bool GATHER> __global__ __launch_bounds__(256) void k_demux_rows(const uint8_t* __restrict__ frames, const int* __restrict__ frame_type,
                                                                         const int* __restrict__ row_frame, const int* __restrict__ n_rows, int n,
                                                                         PiecesLut lut, int row_u, int rows_per_wave, unsigned inv_row_u,
                                                                         uint8_t* __restrict__ rows, int* __restrict__ valid) {
    const long long have = GATHER ? (long long)*n_rows : (long long)n;
    demux_core::rows_thread<GATHER>(blockIdx.x, threadIdx.x, frames, frame_type, row_frame, have, lut, row_u, rows_per_wave, inv_row_u, rows, valid);
}

// the stream, the rule's bitmaps (RefRule::kMaps / TolRule::kMaps) and the frame list
size_t lds_bytes(int maps, int max_bits, int max_frames) { return (size_t)stream_words(max_bits) * (1 + maps) * sizeof(uint32_t) + (size_t)max_frames * sizeof(FrameRec); }

}  // namespace

struct tetra_bsync {
    int n_channels, max_bits, max_frames, device;
    DevMem<State> d_state;
    DevMem<uint8_t> d_carry;
    // the tolerant lock (include/ext/tetra_sync_tol.h): off = the reference's rule and its kernels
    bool tolerant = false;
    Tolerance tol = { 0, 0, 1 };
    DevMem<int32_t> d_miss;           // [C] consecutive LOCKED frames without a candidate (allocated by the first switch to the tolerant rule)
    // the hand-over (include/ext/tetra_handover.h): with the fields, the ASSIST-capable kernels
    DevMem<Assist> d_assist;          // [C] (allocated by the handle's first hand-over, retune_impl::bsync_assist)
};

extern "C" {

int tetra_bsync_create(int n_channels, int max_bits, int device, tetra_bsync_t** out) {
    if (!out || n_channels < 1 || max_bits < 1 || max_bits > kMaxBitsLimit) return TETRA_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    if (device >= ndev) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_HIP;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) return TETRA_ERR_HIP;
    tetra_bsync* h = new tetra_bsync{ n_channels, max_bits, (kBuf + max_bits) / kTs + 2, device };
    if (lds_bytes(RefRule::kMaps, max_bits, h->max_frames) > 160 * 1024 - 64) { delete h; return TETRA_ERR_UNSUPPORTED; }
    if (h->d_state.reserve(sizeof(State) * n_channels) != hipSuccess || h->d_carry.reserve((size_t)kBuf * n_channels) != hipSuccess) {
        delete h;
        return TETRA_ERR_NOMEM;
    }
    // the attribute belongs to the kernel, not to the handle: always raise it to the ceiling so that handles of different
    // sizes can coexist
    for (const void* k : { reinterpret_cast<const void*>(k_burst_sync<false>), reinterpret_cast<const void*>(k_burst_sync<true>),
                           reinterpret_cast<const void*>(k_burst_sync_tol<false>), reinterpret_cast<const void*>(k_burst_sync_tol<true>) })
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64) != hipSuccess) {
            delete h;
            return TETRA_ERR_HIP;
        }
    *out = h;
    return tetra_bsync_reset(h);
}

int tetra_bsync_destroy(tetra_bsync_t* h) {
    if (!h) return TETRA_ERR_ARG;
    delete h;
    return TETRA_OK;
}

int tetra_bsync_reset(tetra_bsync_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_HIP;
    if (hipMemset(h->d_state, 0, sizeof(State) * h->n_channels) != hipSuccess ||
        hipMemset(h->d_carry, 0, (size_t)kBuf * h->n_channels) != hipSuccess ||
        (h->d_miss.get() && hipMemset(h->d_miss, 0, sizeof(int32_t) * h->n_channels) != hipSuccess) ||
        (h->d_assist.get() && hipMemset(h->d_assist, 0, sizeof(Assist) * h->n_channels) != hipSuccess))
        return TETRA_ERR_HIP;
    return TETRA_OK;
}

int tetra_bsync_set_tolerance(tetra_bsync_t* h, const tetra_bsync_tolerance_t* tol) {
    if (!h) return TETRA_ERR_ARG;
    const Tolerance t = tol ? Tolerance{ tol->tol_norm, tol->tol_sync, tol->max_miss } : Tolerance{ 0, 0, 1 };
    if (!tolerance_valid(t)) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok || hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    // the counters exist from the first switch to the tolerant rule on: a handle that never leaves the reference's rule allocates what it
    // always did
    if (tol && !h->d_miss.get() && h->d_miss.reserve(sizeof(int32_t) * h->n_channels) != hipSuccess) return TETRA_ERR_NOMEM;
    if (h->d_miss.get() && hipMemset(h->d_miss, 0, sizeof(int32_t) * h->n_channels) != hipSuccess) return TETRA_ERR_HIP;
    h->tolerant = tol != nullptr;
    h->tol = t;
    return TETRA_OK;
}

int tetra_bsync_get_misses(tetra_bsync_t* h, int first, int count, int32_t* out) {
    if (!h || !out || first < 0 || count < 0 || first + (long long)count > h->n_channels) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok || hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    if (!h->d_miss.get()) {          // never tolerant: nothing was ever counted
        for (int i = 0; i < count; i++) out[i] = 0;
        return TETRA_OK;
    }
    if (count && hipMemcpy(out, h->d_miss + first, sizeof(int32_t) * count, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    return TETRA_OK;
}

int tetra_bsync_max_frames(tetra_bsync_t* h) { return h ? h->max_frames : TETRA_ERR_ARG; }

}  // extern "C"

// The state and the bit buffer tetra_bsync_reset clears, for the stream-ordered reset of listed channels (tetra_retune.hip)
int retune_impl::bsync_view(tetra_bsync_t* h, retune::BsyncView* v) {
    if (!h || !v) return TETRA_ERR_ARG;
    static_assert(sizeof(State) % 4 == 0 && kBuf % 4 == 0, "reset in 32-bit words");
    v->state = reinterpret_cast<uint32_t*>(h->d_state.get()); v->state_words = (int32_t)(sizeof(State) / 4);
    v->carry = reinterpret_cast<uint32_t*>(h->d_carry.get()); v->carry_words = kBuf / 4;
    return TETRA_OK;
}
// ... and the per-channel tables where they are, for the receive chain's description of them (rx_handle.hpp)
int retune_impl::bsync_tables(tetra_bsync_t* h, BsyncTables* t) {
    if (!h || !t) return TETRA_ERR_ARG;
    static_assert(sizeof(State) == sizeof(tetra_bsync_state_t), "state layout");
    *t = { reinterpret_cast<tetra_bsync_state_t*>(h->d_state.get()), h->d_miss.get(), h->tolerant, h->d_assist.get() };
    return TETRA_OK;
}

// The hand-over's per-channel fields: allocated and zeroed by the first call (which waits for the device, once), and from then on the
// handle launches the ASSIST-capable kernels.
int retune_impl::bsync_assist(tetra_bsync_t* h, void** out) {
    if (!h || !out) return TETRA_ERR_ARG;
    if (!h->d_assist.get()) {
        DevMem<Assist> mem;
        if (mem.reserve(sizeof(Assist) * h->n_channels) != hipSuccess) return TETRA_ERR_NOMEM;
        for (const void* k : { reinterpret_cast<const void*>(k_burst_sync_assist<false>), reinterpret_cast<const void*>(k_burst_sync_assist<true>),
                               reinterpret_cast<const void*>(k_burst_sync_tol_assist<false>), reinterpret_cast<const void*>(k_burst_sync_tol_assist<true>) })
            if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64) != hipSuccess) return TETRA_ERR_HIP;
        if (hipMemset(mem, 0, sizeof(Assist) * h->n_channels) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
        h->d_assist = std::move(mem);
    }
    *out = h->d_assist.get();
    return TETRA_OK;
}

namespace {
template <bool PACKED> int bsync_launch(tetra_bsync_t* h, const uint8_t* d_bits, int bits_stride, const int32_t* d_n_bits, void* d_frames,
                                        int32_t* d_frame_type, uint32_t* d_frame_bitnum, int32_t* d_n_frames, void* hip_stream) {
    if (!h || !d_bits || !d_n_bits || !d_frames || !d_frame_type || !d_frame_bitnum || !d_n_frames) return TETRA_ERR_ARG;
    if (bits_stride < 4) return TETRA_ERR_ARG;
    if (bits_stride < h->max_bits) return TETRA_ERR_SIZE;      // rows must be able to hold the max_bits the handle was sized for
    if ((bits_stride & 3) || ((uintptr_t)d_bits & 3) || ((uintptr_t)d_frames & 3)) return TETRA_ERR_ALIGN;
    if (h->d_assist.get() && h->tolerant)
        hipLaunchKernelGGL(k_burst_sync_tol_assist<PACKED>, dim3(h->n_channels), dim3(kThreadsBS), lds_bytes(TolRule::kMaps, h->max_bits, h->max_frames),
                           static_cast<hipStream_t>(hip_stream), d_bits, bits_stride, d_n_bits, h->max_bits, h->max_frames, h->d_state,
                           h->d_carry, static_cast<uint8_t*>(d_frames), d_frame_type, d_frame_bitnum, d_n_frames, h->tol, h->d_miss, h->d_assist);
    else if (h->d_assist.get())
        hipLaunchKernelGGL(k_burst_sync_assist<PACKED>, dim3(h->n_channels), dim3(kThreadsBS), lds_bytes(RefRule::kMaps, h->max_bits, h->max_frames),
                           static_cast<hipStream_t>(hip_stream), d_bits, bits_stride, d_n_bits, h->max_bits, h->max_frames, h->d_state,
                           h->d_carry, static_cast<uint8_t*>(d_frames), d_frame_type, d_frame_bitnum, d_n_frames, h->d_assist);
    else if (h->tolerant)
        hipLaunchKernelGGL(k_burst_sync_tol<PACKED>, dim3(h->n_channels), dim3(kThreadsBS), lds_bytes(TolRule::kMaps, h->max_bits, h->max_frames),
                           static_cast<hipStream_t>(hip_stream), d_bits, bits_stride, d_n_bits, h->max_bits, h->max_frames, h->d_state,
                           h->d_carry, static_cast<uint8_t*>(d_frames), d_frame_type, d_frame_bitnum, d_n_frames, h->tol, h->d_miss);
    else
        hipLaunchKernelGGL(k_burst_sync<PACKED>, dim3(h->n_channels), dim3(kThreadsBS), lds_bytes(RefRule::kMaps, h->max_bits, h->max_frames),
                           static_cast<hipStream_t>(hip_stream), d_bits, bits_stride, d_n_bits, h->max_bits, h->max_frames, h->d_state,
                           h->d_carry, static_cast<uint8_t*>(d_frames), d_frame_type, d_frame_bitnum, d_n_frames);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}
}  // namespace

extern "C" {

int tetra_bsync_process_device(tetra_bsync_t* h, const uint8_t* d_bits, int bits_stride, const int32_t* d_n_bits, uint8_t* d_frames,
                               int32_t* d_frame_type, uint32_t* d_frame_bitnum, int32_t* d_n_frames, void* hip_stream) {
    return bsync_launch<false>(h, d_bits, bits_stride, d_n_bits, d_frames, d_frame_type, d_frame_bitnum, d_n_frames, hip_stream);
}

int tetra_bsync_process_packed_device(tetra_bsync_t* h, const uint8_t* d_bits, int bits_stride, const int32_t* d_n_bits,
                                      uint32_t* d_frames_packed, int32_t* d_frame_type, uint32_t* d_frame_bitnum, int32_t* d_n_frames,
                                      void* hip_stream) {
    return bsync_launch<true>(h, d_bits, bits_stride, d_n_bits, d_frames_packed, d_frame_type, d_frame_bitnum, d_n_frames, hip_stream);
}

int tetra_bsync_process(tetra_bsync_t* h, const uint8_t* bits, int bits_stride, const int32_t* n_bits, uint8_t* frames,
                        int32_t* frame_type, uint32_t* frame_bitnum, int32_t* n_frames) {
    if (!h || !bits || !n_bits || !frames || !frame_type || !frame_bitnum || !n_frames) return TETRA_ERR_ARG;
    if (bits_stride < 4 || (bits_stride & 3)) return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_HIP;
    const int C = h->n_channels, F = h->max_frames;
    DevMem<uint8_t> d_bits, d_frames;
    DevMem<int32_t> d_n, d_ft, d_nf;
    DevMem<uint32_t> d_fb;
    if (d_bits.reserve((size_t)C * bits_stride) != hipSuccess || d_frames.reserve((size_t)C * F * TETRA_FRAME_STRIDE) != hipSuccess ||
        d_n.reserve(sizeof(int32_t) * C) != hipSuccess || d_ft.reserve(sizeof(int32_t) * C * F) != hipSuccess ||
        d_fb.reserve(sizeof(uint32_t) * C * F) != hipSuccess || d_nf.reserve(sizeof(int32_t) * C) != hipSuccess)
        return TETRA_ERR_NOMEM;
    if (hipMemcpy(d_bits, bits, (size_t)C * bits_stride, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_n, n_bits, sizeof(int32_t) * C, hipMemcpyHostToDevice) != hipSuccess)
        return TETRA_ERR_HIP;
    const int rc = tetra_bsync_process_device(h, d_bits, bits_stride, d_n, d_frames, d_ft, d_fb, d_nf, nullptr);
    if (rc != TETRA_OK) return rc;
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(frames, d_frames, (size_t)C * F * TETRA_FRAME_STRIDE, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(frame_type, d_ft, sizeof(int32_t) * C * F, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(frame_bitnum, d_fb, sizeof(uint32_t) * C * F, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(n_frames, d_nf, sizeof(int32_t) * C, hipMemcpyDeviceToHost) != hipSuccess)
        return TETRA_ERR_HIP;
    return TETRA_OK;
}

int tetra_bsync_get_state(tetra_bsync_t* h, int first, int count, tetra_bsync_state_t* out) {
    if (!h || !out || first < 0 || count < 0 || first + count > h->n_channels) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok || hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    static_assert(sizeof(State) == sizeof(tetra_bsync_state_t), "state layout");
    if (count && hipMemcpy(out, h->d_state + first, sizeof(State) * count, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    return TETRA_OK;
}

}  // extern "C"

namespace {
// the argument rules of both demultiplexers behind their null / range checks: the longest block of the kind fits a row; alignment
template <bool PACKED> int demux_check(const uint8_t* d_frames, int tpsap, int blk_num, const uint8_t* d_rows, int row_stride) {
    int longest = 0;
    for (int t : { TETRA_TRAIN_SYNC, TETRA_TRAIN_NORM_1, TETRA_TRAIN_NORM_2 }) {
        const Pieces p = pieces_for(t, tpsap, blk_num);
        longest = p.len0 + p.len1 > longest ? p.len0 + p.len1 : longest;
    }
    if (longest == 0) return TETRA_ERR_ARG;                      // no burst type carries (tpsap, blk_num)
    if (row_stride < longest) return TETRA_ERR_SIZE;
    if ((row_stride & 3) || ((uintptr_t)d_rows & 3)) return TETRA_ERR_ALIGN;
    if (PACKED && ((uintptr_t)d_frames & 3)) return TETRA_ERR_ALIGN;          // packed frames are read as 32-bit words
    return TETRA_OK;
}

template <bool PACKED> int demux_launch(const void* d_frames_v, const int32_t* d_frame_type, int n, int tpsap, int blk_num, uint8_t* d_rows,
                                        int row_stride, int32_t* d_valid, void* hip_stream) {
    const uint8_t* d_frames = static_cast<const uint8_t*>(d_frames_v);
    if (!d_frames || !d_frame_type || !d_rows || !d_valid || n < 0 || tpsap < 0 || tpsap > 5) return TETRA_ERR_ARG;
    if (n == 0) return TETRA_OK;
    TETRA_TRY(demux_check<PACKED>(d_frames, tpsap, blk_num, d_rows, row_stride));
    const bool wide = !(row_stride & 7) && !((uintptr_t)d_rows & 7);
    if (demux_core::use_rows_kernel(PACKED, wide, row_stride)) {           // whole rows per wavefront (k_demux_rows)
        const int row_u = row_stride >> 3, rpw = 64 / row_u;
        hipLaunchKernelGGL((k_demux_rows<false>), dim3((unsigned)demux_core::rows_grid(n, row_stride)), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_frames,
                           d_frame_type, nullptr, nullptr, n, lut_for(tpsap, blk_num), row_u, rpw, (unsigned)((65536 + row_u - 1) / row_u), d_rows, d_valid);
        return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
    }
    const dim3 grid((unsigned)demux_core::units_grid(n, row_stride, wide));
    if (wide) hipLaunchKernelGGL((k_burst_demux<PACKED, true>), grid, dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_frames, d_frame_type, n,
                                 tpsap, blk_num, d_rows, row_stride, d_valid);
    else hipLaunchKernelGGL((k_burst_demux<PACKED, false>), grid, dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_frames, d_frame_type, n,
                            tpsap, blk_num, d_rows, row_stride, d_valid);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

template <bool PACKED> int demux_compact_launch(const void* d_frames_v, const int32_t* d_frame_type, int n, int tpsap, int blk_num,
                                                uint8_t* d_rows, int row_stride, int32_t* d_row_frame, int32_t* d_n_rows, void* hip_stream) {
    const uint8_t* d_frames = static_cast<const uint8_t*>(d_frames_v);
    if (!d_frames || !d_frame_type || !d_rows || !d_row_frame || !d_n_rows || n < 0) return TETRA_ERR_ARG;
    if (tpsap < 0 || tpsap > 5) return TETRA_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (n == 0) return hipMemsetAsync(d_n_rows, 0, sizeof(int32_t), s) == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
    TETRA_TRY(demux_check<PACKED>(d_frames, tpsap, blk_num, d_rows, row_stride));
    // the per-block counts / offsets of the three list passes live in the head of the row buffer itself (4 bytes per 256 frames of a
    // buffer that holds at least 30 bytes per frame; 4-byte aligned): the gather, which overwrites it, runs after their last reader in
    // stream order.  (Until round 5 a stream-ordered allocation per call: every so often the pool gave its memory back in between and
    // one call took milliseconds.)
    lists_launch<1>(CarriesKind{ d_frame_type, tpsap, blk_num }, n, 1, reinterpret_cast<int*>(d_rows), d_row_frame, d_n_rows, nullptr, s);
    const bool wide = !(row_stride & 7) && !((uintptr_t)d_rows & 7);
    const dim3 grid((unsigned)demux_core::units_grid(n, row_stride, wide));
    if (demux_core::use_rows_kernel(PACKED, wide, row_stride)) {           // whole rows per wavefront (k_demux_rows), sized for the worst case of n rows
        const int row_u = row_stride >> 3, rpw = 64 / row_u;
        hipLaunchKernelGGL((k_demux_rows<true>), dim3((unsigned)demux_core::rows_grid(n, row_stride)), dim3(256), 0, s, d_frames, d_frame_type, d_row_frame, d_n_rows, n,
                           lut_for(tpsap, blk_num), row_u, rpw, (unsigned)((65536 + row_u - 1) / row_u), d_rows, nullptr);
    } else if (wide) hipLaunchKernelGGL((k_demux_gather<PACKED, true>), grid, dim3(256), 0, s, d_frames, d_frame_type, d_row_frame, d_n_rows, n, tpsap,
                                 blk_num, d_rows, row_stride);
    else hipLaunchKernelGGL((k_demux_gather<PACKED, false>), grid, dim3(256), 0, s, d_frames, d_frame_type, d_row_frame, d_n_rows, n, tpsap,
                            blk_num, d_rows, row_stride);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}
}  // namespace

extern "C" {

int tetra_burst_demux_device(const uint8_t* d_frames, const int32_t* d_frame_type, int n, int tpsap, int blk_num, uint8_t* d_rows,
                             int row_stride, int32_t* d_valid, void* hip_stream) {
    return demux_launch<false>(d_frames, d_frame_type, n, tpsap, blk_num, d_rows, row_stride, d_valid, hip_stream);
}
int tetra_burst_demux_packed_device(const uint32_t* d_frames_packed, const int32_t* d_frame_type, int n, int tpsap, int blk_num,
                                    uint8_t* d_rows, int row_stride, int32_t* d_valid, void* hip_stream) {
    return demux_launch<true>(d_frames_packed, d_frame_type, n, tpsap, blk_num, d_rows, row_stride, d_valid, hip_stream);
}
int tetra_burst_demux_compact_device(const uint8_t* d_frames, const int32_t* d_frame_type, int n, int tpsap, int blk_num,
                                     uint8_t* d_rows, int row_stride, int32_t* d_row_frame, int32_t* d_n_rows, void* hip_stream) {
    return demux_compact_launch<false>(d_frames, d_frame_type, n, tpsap, blk_num, d_rows, row_stride, d_row_frame, d_n_rows, hip_stream);
}
int tetra_burst_demux_compact_packed_device(const uint32_t* d_frames_packed, const int32_t* d_frame_type, int n, int tpsap, int blk_num,
                                            uint8_t* d_rows, int row_stride, int32_t* d_row_frame, int32_t* d_n_rows, void* hip_stream) {
    return demux_compact_launch<true>(d_frames_packed, d_frame_type, n, tpsap, blk_num, d_rows, row_stride, d_row_frame, d_n_rows, hip_stream);
}

int tetra_burst_index_device(const int32_t* d_frame_type, int n, int frames_per_channel, int32_t* d_lists, int32_t* d_counts,
                             int32_t* d_chan_first, int32_t* d_work, void* hip_stream) {
    if (!d_counts || n < 0) return TETRA_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (n == 0) return hipMemsetAsync(d_counts, 0, sizeof(int32_t) * TETRA_N_LISTS, s) == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;      // (no frames: nothing else is touched)
    if (!d_frame_type || !d_lists || !d_work) return TETRA_ERR_ARG;
    if (d_chan_first && (frames_per_channel < 1 || n % frames_per_channel)) return TETRA_ERR_ARG;
    lists_launch<TETRA_N_LISTS>(ListMask{ d_frame_type }, n, d_chan_first ? frames_per_channel : 1, d_work, d_lists, d_counts, d_chan_first, s);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

}  // extern "C"
