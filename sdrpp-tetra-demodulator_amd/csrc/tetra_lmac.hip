// tetra_lmac.hip -- batched lower-MAC channel decoding (include/tetra_lmac.h), bit-exact with the reference's
// tp_sap_udata_ind() decoding chain (src/decoder/src/lower_mac/tetra_lower_mac.c:181-236).
//
// One 64-lane workgroup (one wavefront) decodes 64 blocks, one block per lane.  Everything a lane computes is lane-level code in
// lmac_core.hpp (soft_core.hpp for the soft front end) -- pack_units / staged_row, descramble_chunk, the block front ends (frame_lookup,
// load_frame, frame_hard_block, byte_row_block, soft_block: one function per source, called by the decode kernel and by the rescue
// behind it alike), decode_hard / decode_soft, write_rows -- where tests/emul runs the same source on the host; this file holds the
// kernels' LDS and global-memory accessors, the barriers, and the host side: every frame entry point is lmac_impl::decode_frames
// (lmac_impl.hpp) with the options its signature can express.
//   1. front end -> the descrambled type-4 bits of the lane's block as packed words in LDS, [word][lane]:
//      * from PACKED FRAMES (k_lmac_frames, round 6): the lane reads its frame (four 16-byte loads), cuts the kind's one or two bit
//        ranges out with funnel shifts and XORs whole words of its scrambling sequence (linear in the code: four rows of a 64 KB
//        table indexed by the code's bytes);
//      * from byte rows of plain bits (k_lmac_decode; every byte 0 / 1): the workgroup reads its 64 rows as one contiguous run,
//        8 bytes per lane, packs them to bits through LDS, each lane takes its row's words, then the same;
//      * from byte rows with any other byte value anywhere in the workgroup's 64 rows (erasures), or rows that are not 8-byte
//        aligned: the byte route -- rows staged through LDS in coalesced 64-bit chunks, an LFSR step and a three-way classification
//        (0 / erasure 0xff / 1) per byte, soft classes 2 bits per type-4 bit in LDS;
//   2. forward recursion: 16 path metrics in 8 registers (packed int16: states i and i + 8), the three soft values of a step pair
//      gathered from LDS at the deinterleaved positions (wave-uniform addresses), a butterfly = add, subtract, maximum, difference
//      with the halves picked by operand modifiers (no moves), the 2 x 16 decision bits of a step pair gathered with byte permutes
//      and stored as one dword to a global scratch laid out [workgroup][step pair][lane] (one 256-byte line per pair; written
//      once, read once, normally from L2 / MALL): 99 vector instructions per step pair;
//   3. traceback from the scratch (the addresses do not depend on the surviving state, only the bit picked does, so the loads
//      pipeline) with the CRC16 folded in (affine in the message: one AND + XOR per bit with a wave-uniform constant), decoded bits
//      packed 16 per ushort into LDS [half][lane];
//   4. the 64 decoded rows are written back with coalesced 8-byte stores, 8 bits -> 8 bytes per lane.
// A launch that is asked for channel bit-error counts (include/ext/tetra_biterr.h) runs the COUNT instantiation of its kernel: between 3 and
// 4 each lane encodes its decoded bits again and holds them against its block, both still in LDS (lmac_core.hpp reencode_errors).
// The work is integer add / compare / select: bound by vector issue.
#include <hip/hip_runtime.h>

#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/tetra_aach.h"
#include "../../include/ext/tetra_biterr.h"
#include "../../include/ext/tetra_list.h"
#include "../../include/ext/tetra_aach_soft.h"
#include "../../include/ext/tetra_soft.h"
#include "../../include/ext/tetra_tch.h"
#include "../../include/ext/tetra_tch_soft.h"
#include "../../include/ext/tetra_tch_nblk.h"
#include "../../include/tetra_lmac.h"
#include "demux_core.hpp"
#include "compact_core.hpp"
#include "hip_host.hpp"
#include "list_core.hpp"
#include "lmac_core.hpp"
#include "lmac_impl.hpp"
#include "soft_core.hpp"
#include "tch_core.hpp"
#include "tch_soft_core.hpp"
#include "tch_nblk_core.hpp"

namespace {

using namespace tetra_lmac;

constexpr int kOutHalves = kMaxType2 / 16;             // 18
constexpr int kOutPad = 2;                             // outw rows of 66 ushorts = 33 banks: the write-back's column reads do not collide
bool g_force_byte_route = false;                       // tests / A-B: tetra_lmac_debug_force_byte_route
__constant__ CrcInvTable kCrcInvDev = make_crc_inv_table();      // the traceback's backward CRC table; every workgroup copies it to LDS

typedef uint16_t OutW[kOutHalves][kLanes + kOutPad];

// What steps 2-3 (decode_hard, decode_soft) touch besides the lane's type-4 bits: its column of the decoded halves and the backward CRC
// table in LDS, and its decision words in the global scratch, laid out [step pair][lane]
struct LaneIo {
    OutW& outw;
    const uint32_t* crc_inv;
    uint32_t* dec;
    int lane;
    __device__ __forceinline__ void dec_st(int u, uint32_t w) const { dec[u * kLanes] = w; }
    __device__ __forceinline__ uint32_t dec_ld(int u) const { return dec[u * kLanes]; }
    __device__ __forceinline__ void out_st(int h, uint32_t half) const { outw[h][lane] = (uint16_t)half; }
    __device__ __forceinline__ uint32_t tinv(uint32_t off) const { return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(crc_inv) + off); }
};

// the backward CRC table into LDS (4 entries per lane); the caller's next barrier makes it visible
__device__ __forceinline__ void load_crc_inv(uint32_t* crc_inv, int lane) {
#pragma unroll
    for (int k = 0; k < 256 / kLanes; ++k) crc_inv[k * kLanes + lane] = kCrcInvDev.t[k * kLanes + lane];
}

// step 4 (lmac_core.hpp write_rows) from LDS to the workgroup's rows in HBM
__device__ __forceinline__ void write_rows(const OutW& outw, int lane, int rows_here, int type2, uint8_t* __restrict__ out0, int out_stride) {
    tetra_lmac::write_rows(lane, rows_here, type2, rows_wide(out0, out_stride), [&](int h, int q) { return outw[h][q]; },
               [&](int q, int d, demux_core::U2 v) { reinterpret_cast<demux_core::U2*>(out0 + (size_t)q * out_stride)[d] = v; },
               [&](int q, int d, uint32_t v) { reinterpret_cast<uint32_t*>(out0 + (size_t)q * out_stride)[d] = v; });
}

// lane_sequence's rows of the device's sequence table: 16-byte loads
__device__ __forceinline__ auto seq_rows(const uint32_t* __restrict__ seq_tab) {
    return [=](int t, uint32_t byte) { return reinterpret_cast<const uint4*>(seq_tab + ((size_t)t * 256 + byte) * kSeqStride); };
}

// load_frame's 16-byte rows of frame f
__device__ __forceinline__ auto frame_rows(const uint32_t* frames, int f) {
    const uint4* src = reinterpret_cast<const uint4*>(frames + (size_t)f * kFrameWords);
    return [=](int g) { return src[g]; };
}
// soft_block's ring of one channel: aligned words
__device__ __forceinline__ auto ring_of(const uint32_t* ring, uint32_t ring_words, int channel) {
    const uint32_t* chan = ring + (size_t)channel * ring_words;
    return [=](uint32_t w) { return chan[w]; };
}

// The channel bit-error counts (tetra_biterr.h) are an instantiation of each decode kernel: COUNT = true takes where the counts go as a
// trailing parameter pack -- one argument, none otherwise, as k_lmac_bbk takes its table -- so that the instantiation without the option
// has the argument block and the instruction stream it had before the option existed.
template <class T> __device__ __forceinline__ T only_of(T t) { return t; }

template <bool COUNT, class... Biterr>
__global__ __launch_bounds__(kLanes) void k_lmac_decode(const uint8_t* __restrict__ type5, int n_blocks, int in_stride,
                                                        const uint32_t* __restrict__ scramb_init, int fixed_init,
                                                        int type345, int type2, int type1, int a,
                                                        uint8_t* __restrict__ out, int out_stride, int* __restrict__ crc_ok,
                                                        uint32_t* __restrict__ dec_scratch, int dec_pairs,
                                                        const int* __restrict__ n_blocks_dev, const int* __restrict__ init_index,
                                                        const uint32_t* __restrict__ seq_tab, Biterr... biterr_pack) {
    __shared__ uint32_t stage[kLanes][kStageWords];
    __shared__ uint32_t cls[kClsWords + 1][kLanes];
    __shared__ OutW outw;
    __shared__ uint32_t crc_inv[256];
    const int lane = threadIdx.x;
    const int blk0 = blockIdx.x * kLanes;
    const int blk = blk0 + lane;
    if (n_blocks_dev) {           // counted form: the number of rows is a device-side result (compacting demultiplexer)
        const int have = *n_blocks_dev;
        n_blocks = have < n_blocks ? have : n_blocks;
        if (blk0 >= n_blocks) return;
    }
    const int rows_here = min(kLanes, n_blocks - blk0);
    const uint32_t code = (fixed_init || blk >= n_blocks) ? kScrambInitSb1 : scramb_init[init_index ? init_index[blk] : blk];
    uint32_t* dec = dec_scratch + (size_t)blockIdx.x * dec_pairs * kLanes + lane;
    load_crc_inv(crc_inv, lane);

    // 1. front end.  Rows of plain bits: each lane packs its own row (8-byte loads), descrambles whole words and leaves the type-4
    //    bits in LDS (cls rows 0..13 as [word][lane]); the workgroup falls back to the byte route if any of its rows holds another
    //    byte value, or if the rows are not 8-byte aligned.
    bool byte_route = needs_byte_route(seq_tab, type5, in_stride);
    LaneIo io{ outw, crc_inv, dec, lane };
    if (!byte_route) {
        // pack_units: the workgroup reads its rows as one contiguous run.  (Until late in round 6 every lane read its own row with strided
        // 8-byte loads: 64 cache lines per instruction, and with a few waves per CU the lines were evicted before their other 120 bytes
        // were used.)
        const U2* base = reinterpret_cast<const U2*>(type5 + (size_t)blk0 * in_stride);
        uint8_t* sb = reinterpret_cast<uint8_t*>(&stage[0][0]);
        const uint32_t dirty = pack_units(lane, rows_here, in_stride, type345, [&](int u) { return base[u]; },
                                          [&](size_t at, uint8_t byte) { sb[at] = byte; });
        byte_route = __builtin_amdgcn_ballot_w64(dirty != 0) != 0;          // wave-uniform
        __syncthreads();
        if (!byte_route) {
            uint32_t xb[kSeqWords];
            const uint32_t* mine = stage[lane];
            staged_row(type345, [&](int w) { return mine[w]; }, xb);
            descramble_words(type345, code, xb, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w][lane] = word; });
        }
    }
    bool good;
    uint32_t biterr = 0;                      // COUNT: errors | compared << 16 of the lane's block, from its decoded halves and its staged bits
    auto half = [&](int h) { return outw[h][lane]; };
    auto staged = [&](int w) { return cls[w][lane]; };
    if (!byte_route) {
        __syncthreads();
        good = decode_hard<true>(type345, type2, a, staged, io);
        if constexpr (COUNT) biterr = bit_errors_hard<true>(type345, type2, a, half, staged);
    } else {
        // rows -> LDS in chunks of 64 bits per row (coalesced 64-byte segments, 4 rows per load instruction), each lane
        // descrambles its own row chunk by chunk (its LFSR carried in a register) and packs the soft classes
        uint32_t lfsr = code;
        const int row_dw = type345 >> 2;
        for (int c0 = 0; c0 < row_dw; c0 += kChunkDwords) {
#pragma unroll 4
            for (int it = 0; it < kLanes * kChunkDwords / kLanes; ++it) {
                const int q = it * (kLanes / kChunkDwords) + lane / kChunkDwords, d = lane % kChunkDwords;
                uint32_t v = 0;
                if (q < rows_here && c0 + d < row_dw)
                    v = reinterpret_cast<const uint32_t*>(type5 + (size_t)(blk0 + q) * in_stride)[c0 + d];
                stage[q][d] = v;
            }
            __syncthreads();
            lfsr = descramble_chunk(type345 - 4 * c0, lfsr, [&](int d) { return stage[lane][d]; },
                                    [&](int w, uint32_t word) { cls[c0 / 4 + w][lane] = word; });
            __syncthreads();
        }
        good = decode_hard<false>(type345, type2, a, staged, io);
        if constexpr (COUNT) biterr = bit_errors_hard<false>(type345, type2, a, half, staged);
    }
    if (blk < n_blocks) crc_ok[blk] = good;
    if constexpr (COUNT) {
        if (blk < n_blocks) only_of(biterr_pack...)[blk] = biterr;
    }
    __syncthreads();
    write_rows(outw, lane, rows_here, type2, out + (size_t)blk0 * out_stride, out_stride);
}

// ---- straight from packed frames, several kinds per launch (tetra_lmac_decode_frames_device) ----------------------------------
struct DevJob {
    const int* row_frame;
    const int* n_rows_dev;
    const uint32_t* frame_scramb;
    uint8_t* out;
    int* crc_ok;
    tetra_lmac_label_t* labels;
    long long scratch_base;            // first word of the job's decision scratch
    int n_rows, out_stride, first_group, dec_pairs;
    int layout;                        // kLayout*
    int type345, type2, a;
};
struct DevFrames {
    const uint32_t* frames;
    const int* frame_type;
    const uint32_t* bitnum;
    const uint32_t* time_rx;
    const uint32_t* time;
    int frames_per_channel;
    int n_frames;
};
struct JobTable {
    DevJob job[TETRA_LMAC_MAX_JOBS];
    DevFrames src;
    int n;
};
// a row's verdict and, where the job asks for them, its label
__device__ __forceinline__ void write_verdict(const DevJob& J, const DevFrames& src, int blk, int f, bool good) {
    J.crc_ok[blk] = good;
    if (J.labels) {
        tetra_lmac_label_t lb;
        lb.channel = f / src.frames_per_channel;
        lb.frame_slot = f - lb.channel * src.frames_per_channel;
        lb.bitnum = src.bitnum[f];
        lb.tdma_time_rx = src.time_rx[f];
        lb.tdma_time = src.time[f];
        lb.crc_ok = good;
        J.labels[blk] = lb;
    }
}
// The frame kernels' prologue, in two halves around the kernel's own `if (L.blk0 >= L.n_blocks) return;` (as one function that also says
// "nothing to do" it compiles to a materialised predicate and a dozen more instructions per kernel): frame_group finds the workgroup's
// job and rows, frame_of the lane's frame and its scrambling code.
struct FrameLane {
    const DevJob& J;
    int group, blk0, blk, n_blocks, rows_here;
    int f;
    uint32_t code;
};
__device__ __forceinline__ FrameLane frame_group(const JobTable& tab, int lane) {
    int ji = 0;
    for (int i = 1; i < tab.n; ++i) ji = (int)blockIdx.x >= tab.job[i].first_group ? i : ji;
    const DevJob& J = tab.job[ji];
    const int group = (int)blockIdx.x - J.first_group, blk0 = group * kLanes;
    int n_blocks = J.n_rows;
    if (J.n_rows_dev) {           // counted rows: a device-side result (the frame lists)
        const int have = *J.n_rows_dev;
        n_blocks = have < n_blocks ? have : n_blocks;
    }
    return FrameLane{ J, group, blk0, blk0 + lane, n_blocks, min(kLanes, n_blocks - blk0), 0, 0u };
}
__device__ __forceinline__ void frame_of(const JobTable& tab, FrameLane& L) {
    const FrameRef r = frame_lookup(L.J.row_frame[L.blk < L.n_blocks ? L.blk : L.blk0], tab.src.n_frames, L.J.frame_scramb);
    L.f = r.f;
    L.code = r.code;
}
// Where the counts of a frame launch go: per job of the table, NULL = the job does not count (tetra_lmac_decode_frames_biterr_device).
struct BiterrTable { uint32_t* out[TETRA_LMAC_MAX_JOBS]; };
// the workgroup's entry, found as frame_group finds its job (selects over the argument block: indexing it would put it in scratch)
__device__ __forceinline__ uint32_t* job_counts(const JobTable& tab, const BiterrTable& bt) {
    uint32_t* c = bt.out[0];
#pragma unroll
    for (int i = 1; i < TETRA_LMAC_MAX_JOBS; ++i) c = i < tab.n && (int)blockIdx.x >= tab.job[i].first_group ? bt.out[i] : c;
    return c;
}
// A frame kernel's staged block and its decoded halves.  Without counts the halves reuse the block's space once the forward recursion is
// through with it; the counting instantiations hold the decoded block against the staged one, so they keep both.
template <class Staged, bool KEEP> struct BlockLds { union { Staged in; OutW outw; }; };
template <class Staged> struct BlockLds<Staged, true> { Staged in; OutW outw; };
// LDS per workgroup: 3584 (type-4 bits; the decoded halves reuse the space once the forward recursion is through with them) + 1024
// (backward CRC table) = 4608 B <= 5120: LDS never caps the kernel below 8 waves per SIMD -- which matters beside the demodulator:
// the compiler sizes a kernel's register allocation for the occupancy its LDS allows (6992 B -> 6 waves -> 80 registers where 54 are
// used), and next to k_fused's 199-register waves every 8 registers decide how many of this kernel's waves fit a SIMD.
// RM: the instantiation that also knows kLayoutBbkRm -- the AACH's 30 descrambled bits through rm3014_decode (one syndrome, one look-up
// in rm_tab), a lane per block like the pass-through.  Launched only when a job asks for it; <false> is the kernel as it was.
// COUNT: + 2376 (the decoded halves beside the type-4 bits, rounded up to 8) = 6992 B, 23 workgroups per CU; the counting instantiations
// still allocate 50 to 54 registers (the 80 above was a build of its time, not a rule).
template <bool RM, bool COUNT = false, class... Biterr>
__global__ __launch_bounds__(kLanes) void k_lmac_frames(const JobTable tab, uint32_t* __restrict__ dec_scratch,
                                                        const uint32_t* __restrict__ seq_tab, const uint32_t* __restrict__ rm_tab, Biterr... biterr_pack) {
    typedef uint32_t Cls[kSeqWords][kLanes];
    __shared__ BlockLds<Cls, COUNT> sm;
    static_assert(sizeof(OutW) <= sizeof(Cls), "the decoded halves fit the type-4 words' space");
    Cls& cls = sm.in;
    OutW& outw = sm.outw;
    __shared__ uint32_t crc_inv[256];
    const int lane = threadIdx.x;
    FrameLane L = frame_group(tab, lane);
    if (L.blk0 >= L.n_blocks) return;
    frame_of(tab, L);
    const DevJob& J = L.J;
    const int ft = tab.src.frame_type[L.f];
    uint32_t fw[kFrameWords];
    load_frame(frame_rows(tab.src.frames, L.f), fw);
    bool good = true;
    const bool bbk = J.layout == kLayoutBbk || (RM && J.layout == kLayoutBbkRm);
    if (bbk) {
        // TPSAP_T_BBK: the reference only descrambles (tetra_lower_mac.c:231-236): 30 bits -> 30 bytes (+ 2 zero bytes), a row per lane
        const uint32_t x = bbk_bits(fw, ft);
        uint32_t seq = 0;
        lane_sequence(30, L.code, seq_rows(seq_tab), [&](int w, uint32_t word) { seq = w == 0 ? word : seq; });
        uint32_t y = (x ^ seq) & 0xfffffffcu;                // 30 bits, first bit most significant
        uint32_t tail = 0;                                   // row bytes 30, 31
        if (RM && J.layout == kLayoutBbkRm) {
            const Rm3014Word r = rm3014_decode(y >> 2, [&](uint32_t s) { return rm_tab[s]; });
            y = r.word << 2;
            tail = r.dist << 16;
            good = r.dist <= (uint32_t)kRm3014Radius;
        }
        if (L.blk < L.n_blocks) {
            demux_core::U2* dst = reinterpret_cast<demux_core::U2*>(J.out + (size_t)L.blk * J.out_stride);
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[k] = demux_core::U2{ bbk_bytes(y, 2 * k), bbk_bytes(y, 2 * k + 1) | (k == 3 ? tail : 0u) };
        }
    } else {
        frame_hard_block(&J, L.code, fw, [&] { return ft; }, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w][lane] = word; });
        load_crc_inv(crc_inv, lane);
        __syncthreads();
        LaneIo io{ outw, crc_inv, dec_scratch + J.scratch_base + (size_t)L.group * J.dec_pairs * kLanes + lane, lane };
        good = decode_hard<true>(J.type345, J.type2, J.a, [&](int w) { return cls[w][lane]; }, io);
        if constexpr (COUNT) {
            uint32_t* counts = job_counts(tab, only_of(biterr_pack...));            // (workgroup-uniform: a workgroup has one job)
            if (counts) {
                const uint32_t biterr = bit_errors_hard<true>(J.type345, J.type2, J.a, [&](int h) { return outw[h][lane]; }, [&](int w) { return cls[w][lane]; });
                if (L.blk < L.n_blocks) counts[L.blk] = biterr;
            }
        }
    }
    if (L.blk < L.n_blocks) write_verdict(J, tab.src, L.blk, L.f, good);
    if (!bbk) {
        __syncthreads();
        write_rows(outw, lane, L.rows_here, J.type2, J.out + (size_t)L.blk0 * J.out_stride, J.out_stride);
    }
}

// ---- the coded kinds from SOFT values (lmac_impl::FrameOpts::soft: the receive chain's TETRA_RX_FLAG_SOFT) --------------------------
// k_lmac_frames with another front end: where that kernel cuts a block's bits out of the packed frame, this one reads the block's soft
// values from the chain's ring at the frame's absolute bit number, descrambles them by sign and stages them in LDS as bytes
// (soft_core.hpp); the forward recursion takes its branch metrics from those bytes; traceback, backward CRC, verdict, label and row
// write-back are the hard route's, unchanged.
// LDS per workgroup: 27648 (432 staged bytes per lane; the decoded halves reuse the space) + 1024 (backward CRC table) = 28672 B: five
// workgroups = five waves per CU where the hard kernel's 4608 B allow 32, so beside k_fused this launch keeps at most five decoder waves
// on a CU and hides the latency of its ring loads with its own unrolled loads rather than with other waves.
// COUNT: + 2376 (rounded up to 8) = 31056 B, still five workgroups per CU.
template <bool COUNT, class... Biterr>
__global__ __launch_bounds__(kLanes) void k_lmac_frames_soft(const JobTable tab, uint32_t* __restrict__ dec_scratch, const uint32_t* __restrict__ seq_tab,
                                                             const uint32_t* __restrict__ ring, uint32_t ring_words, Biterr... biterr_pack) {
    using namespace tetra_soft;
    typedef uint32_t Soft[kSoftWords][kLanes];
    __shared__ BlockLds<Soft, COUNT> sm;
    __shared__ uint32_t crc_inv[256];
    const int lane = threadIdx.x;
    FrameLane L = frame_group(tab, lane);
    if (L.blk0 >= L.n_blocks) return;
    frame_of(tab, L);
    const DevJob& J = L.J;
    soft_block(&J, L.code, [&] { return tab.src.bitnum[L.f]; }, [&] { return tab.src.frame_type[L.f]; }, seq_rows(seq_tab),
               ring_of(ring, ring_words, L.f / tab.src.frames_per_channel), ring_words, [&](int g, uint32_t word) { sm.in[g][lane] = word; });
    load_crc_inv(crc_inv, lane);
    __syncthreads();
    LaneIo io{ sm.outw, crc_inv, dec_scratch + J.scratch_base + (size_t)L.group * J.dec_pairs * kLanes + lane, lane };
    const bool good = decode_soft(J.type345, J.type2, J.a, [&](int w) { return sm.in[w][lane]; }, io);
    if constexpr (COUNT) {
        uint32_t* counts = job_counts(tab, only_of(biterr_pack...));
        if (counts) {
            const uint32_t biterr = bit_errors_soft(J.type345, J.type2, J.a, [&](int h) { return sm.outw[h][lane]; }, [&](int w) { return sm.in[w][lane]; });
            if (L.blk < L.n_blocks) counts[L.blk] = biterr;
        }
    }
    if (L.blk < L.n_blocks) write_verdict(J, tab.src, L.blk, L.f, good);
    __syncthreads();
    write_rows(sm.outw, lane, L.rows_here, J.type2, J.out + (size_t)L.blk0 * J.out_stride, J.out_stride);
}

// ---- circuit-mode data channels TCH/7.2, TCH/4.8, TCH/2.4 (include/ext/tetra_tch.h; lane code: tch_core.hpp) ---------------------------
// Kernels of their own, so that the kernels above are the code objects they were: the workgroup shape (one wavefront, a block per lane),
// the front ends, the decision scratch [workgroup][step pair][lane] and the row write-back are k_lmac_decode's and k_lmac_frames'; the
// forward recursion takes its branch metrics from up to three generators per step by the kind's schedule, the traceback has no CRC
// beside it, and a launch that counts encodes the decoded bits again with the same schedule.  The kind (generators per step, ng) is
// workgroup-uniform; TCH/7.2 (ng = 0) is descrambling alone: a lane fetches its row's scrambling sequence, the workgroup XORs it onto
// the rows four bytes at a time.
typedef uint16_t TchOutW[tetra_tch::kOutHalves][kLanes + kOutPad];
struct TchIo {
    TchOutW& outw;
    uint32_t* dec;
    int lane;
    __device__ __forceinline__ void dec_st(int u, uint32_t w) const { dec[u * kLanes] = w; }
    __device__ __forceinline__ uint32_t dec_ld(int u) const { return dec[u * kLanes]; }
    __device__ __forceinline__ void out_st(int h, uint32_t half) const { outw[h][lane] = (uint16_t)half; }
    __device__ __forceinline__ uint32_t out_ld(int h) const { return outw[h][lane]; }
};
__device__ __forceinline__ void tch_write_rows(const TchOutW& outw, int lane, int rows_here, int type2, uint8_t* __restrict__ out0, int out_stride) {
    tetra_tch::write_rows(lane, rows_here, type2, rows_wide(out0, out_stride), [&](int h, int q) { return outw[h][q]; },
                          [&](int q, int d, demux_core::U2 v) { reinterpret_cast<demux_core::U2*>(out0 + (size_t)q * out_stride)[d] = v; },
                          [&](int q, int d, uint32_t v) { reinterpret_cast<uint32_t*>(out0 + (size_t)q * out_stride)[d] = v; });
}
// LDS per workgroup: 4352 (staging) + 7168 (the block as bits or soft classes) + 2508 (decoded halves) = 14028 B.
// packed_ok = 0: every row through the byte route (tetra_lmac_debug_force_byte_route); biterr_out NULL: no counts.
__global__ __launch_bounds__(kLanes) void k_tch_rows(const uint8_t* __restrict__ type5, int n_blocks, int in_stride,
                                                     const uint32_t* __restrict__ scramb_init, int ng, int type2,
                                                     uint8_t* __restrict__ out, int out_stride,
                                                     uint32_t* __restrict__ dec_scratch, int dec_pairs,
                                                     const int* __restrict__ n_blocks_dev, const int* __restrict__ init_index,
                                                     const uint32_t* __restrict__ seq_tab, int packed_ok, uint32_t* __restrict__ biterr_out) {
    __shared__ uint32_t stage[kLanes][kStageWords];
    __shared__ uint32_t cls[kClsWords + 1][kLanes];
    __shared__ TchOutW outw;
    const int lane = threadIdx.x;
    const int blk0 = blockIdx.x * kLanes;
    const int blk = blk0 + lane;
    if (n_blocks_dev) {
        const int have = *n_blocks_dev;
        n_blocks = have < n_blocks ? have : n_blocks;
        if (blk0 >= n_blocks) return;
    }
    const int rows_here = min(kLanes, n_blocks - blk0);
    const uint32_t code = blk >= n_blocks ? kScrambInitSb1 : scramb_init[init_index ? init_index[blk] : blk];
    constexpr int type345 = tetra_tch::kType345;
    if (ng == 0) {
        lane_sequence(type345, code, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w][lane] = word; });
        __syncthreads();
        tetra_tch::passthrough_rows(lane, rows_here, [&](int w, int q) { return cls[w][q]; },
                                    [&](int q, int d) { return reinterpret_cast<const uint32_t*>(type5 + (size_t)(blk0 + q) * in_stride)[d]; },
                                    [&](int q, int d, uint32_t v) { reinterpret_cast<uint32_t*>(out + (size_t)(blk0 + q) * out_stride)[d] = v; });
        return;
    }
    // the front end of k_lmac_decode
    bool byte_route = needs_byte_route(packed_ok ? seq_tab : nullptr, type5, in_stride);
    if (!byte_route) {
        const U2* base = reinterpret_cast<const U2*>(type5 + (size_t)blk0 * in_stride);
        uint8_t* sb = reinterpret_cast<uint8_t*>(&stage[0][0]);
        const uint32_t dirty = pack_units(lane, rows_here, in_stride, type345, [&](int u) { return base[u]; },
                                          [&](size_t at, uint8_t byte) { sb[at] = byte; });
        byte_route = __builtin_amdgcn_ballot_w64(dirty != 0) != 0;          // wave-uniform
        __syncthreads();
        if (!byte_route) {
            uint32_t xb[kSeqWords];
            const uint32_t* mine = stage[lane];
            staged_row(type345, [&](int w) { return mine[w]; }, xb);
            descramble_words(type345, code, xb, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w][lane] = word; });
        }
    }
    TchIo io{ outw, dec_scratch + (size_t)blockIdx.x * dec_pairs * kLanes + lane, lane };
    auto staged = [&](int w) { return cls[w][lane]; };
    uint32_t biterr;
    if (!byte_route) {
        __syncthreads();
        biterr = tetra_tch::decode_lane<true>(ng, type2, biterr_out != nullptr, staged, io);
    } else {
        uint32_t lfsr = code;
        const int row_dw = type345 >> 2;
        for (int c0 = 0; c0 < row_dw; c0 += kChunkDwords) {
#pragma unroll 4
            for (int it = 0; it < kLanes * kChunkDwords / kLanes; ++it) {
                const int q = it * (kLanes / kChunkDwords) + lane / kChunkDwords, d = lane % kChunkDwords;
                uint32_t v = 0;
                if (q < rows_here && c0 + d < row_dw)
                    v = reinterpret_cast<const uint32_t*>(type5 + (size_t)(blk0 + q) * in_stride)[c0 + d];
                stage[q][d] = v;
            }
            __syncthreads();
            lfsr = descramble_chunk(type345 - 4 * c0, lfsr, [&](int d) { return stage[lane][d]; },
                                    [&](int w, uint32_t word) { cls[c0 / 4 + w][lane] = word; });
            __syncthreads();
        }
        biterr = tetra_tch::decode_lane<false>(ng, type2, biterr_out != nullptr, staged, io);
    }
    if (biterr_out && blk < n_blocks) biterr_out[blk] = biterr;
    __syncthreads();
    tch_write_rows(outw, lane, rows_here, type2, out + (size_t)blk0 * out_stride, out_stride);
}

// The TCH jobs of a frame launch: k_lmac_frames' prologue, the SCH/F cut of the frame, verdict 1 and the label; counts.out[job] NULL: the
// job does not count.  LDS per workgroup: 3584 (type-4 bits) + 2508 (decoded halves) = 6092 B.
__global__ __launch_bounds__(kLanes) void k_tch_frames(const JobTable tab, uint32_t* __restrict__ dec_scratch, const uint32_t* __restrict__ seq_tab,
                                                       const BiterrTable counts_tab) {
    __shared__ uint32_t cls[kSeqWords][kLanes];
    __shared__ TchOutW outw;
    const int lane = threadIdx.x;
    FrameLane L = frame_group(tab, lane);
    if (L.blk0 >= L.n_blocks) return;
    frame_of(tab, L);
    const DevJob& J = L.J;
    const int ft = tab.src.frame_type[L.f];
    uint32_t fw[kFrameWords];
    load_frame(frame_rows(tab.src.frames, L.f), fw);
    frame_hard_block(&J, L.code, fw, [&] { return ft; }, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w][lane] = word; });
    if (L.blk < L.n_blocks) write_verdict(J, tab.src, L.blk, L.f, true);
    const int ng = tetra_tch::ng_of_type2(J.type2);
    uint8_t* out0 = J.out + (size_t)L.blk0 * J.out_stride;
    __syncthreads();
    if (ng == 0) {
        tetra_tch::passthrough_rows(lane, L.rows_here, [&](int w, int q) { return cls[w][q]; }, [&](int, int) { return 0u; },
                                    [&](int q, int d, uint32_t v) { reinterpret_cast<uint32_t*>(out0 + (size_t)q * J.out_stride)[d] = v; });
        return;
    }
    TchIo io{ outw, dec_scratch + J.scratch_base + (size_t)L.group * J.dec_pairs * kLanes + lane, lane };
    uint32_t* counts = job_counts(tab, counts_tab);            // (workgroup-uniform: a workgroup has one job)
    const uint32_t biterr = tetra_tch::decode_lane<true>(ng, J.type2, counts != nullptr, [&](int w) { return cls[w][lane]; }, io);
    if (counts && L.blk < L.n_blocks) counts[L.blk] = biterr;
    __syncthreads();
    tch_write_rows(outw, lane, L.rows_here, J.type2, out0, J.out_stride);
}

// ---- the coded data channels from SOFT values (include/ext/tetra_tch_soft.h; lane code: tch_soft_core.hpp) ----------------------------------
// The two kernels above with the soft front end of k_lmac_frames_soft: a lane's block is 432 staged bytes in LDS, the forward recursion
// takes raw soft values by the kind's schedule; traceback, counts, scratch [workgroup][step pair][lane] and row write-back are the hard
// siblings'.  One wavefront per workgroup, a block per lane; ng (2 or 3) is workgroup-uniform.
// LDS per workgroup, k_tch_rows_soft: 28080 (108 staged words x 65: the rows arrive transposed, see below) + 2508 (decoded halves) =
// 30588 B; k_tch_frames_soft: 27648 + 2508 = 30156 B.  Either way five workgroups = five waves per CU of 160 KB, as k_lmac_frames_soft
// has (beside k_fused the decoder's launches fill what LDS is left, 64-thread workgroups).  Letting the halves reuse the staging
// space would save 2508 B and still give five, so they keep a space of their own and the counts need no second instantiation.
typedef uint32_t TchSoftRows[tetra_tch_soft::kSoftWords][kLanes + 1];
typedef uint32_t TchSoftCols[tetra_tch_soft::kSoftWords][kLanes];

// int8 byte rows.  The workgroup copies its rows into LDS as they lie in memory, a row per iteration and a dword per lane (coalesced:
// 256 bytes an instruction, where a lane reading its own row would touch 64 cache lines an instruction), transposed into [word][row]; the
// odd pitch of 65 words keeps both the transposing writes (bank 65 d + q) and the lanes' column reads (bank q) free of conflicts.  Each lane then
// descrambles its own column in place.  Rows past rows_here are staged as zeros.  biterr_out NULL: no counts.
__global__ __launch_bounds__(kLanes) void k_tch_rows_soft(const int8_t* __restrict__ soft5, int n_blocks, int in_stride,
                                                          const uint32_t* __restrict__ scramb_init, int ng, int type2,
                                                          uint8_t* __restrict__ out, int out_stride,
                                                          uint32_t* __restrict__ dec_scratch, int dec_pairs,
                                                          const int* __restrict__ n_blocks_dev, const int* __restrict__ init_index,
                                                          const uint32_t* __restrict__ seq_tab, uint32_t* __restrict__ biterr_out) {
    using namespace tetra_tch_soft;
    __shared__ TchSoftRows in;
    __shared__ TchOutW outw;
    const int lane = threadIdx.x;
    const int blk0 = blockIdx.x * kLanes;
    const int blk = blk0 + lane;
    if (n_blocks_dev) {
        const int have = *n_blocks_dev;
        n_blocks = have < n_blocks ? have : n_blocks;
    }
    if (blk0 >= n_blocks) return;
    const int rows_here = min(kLanes, n_blocks - blk0);
    const uint32_t code = blk >= n_blocks ? kScrambInitSb1 : scramb_init[init_index ? init_index[blk] : blk];
#pragma unroll 4
    for (int q = 0; q < kLanes; ++q) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(soft5 + (size_t)(blk0 + q) * in_stride);
#pragma unroll
        for (int d = lane; d < kSoftWords; d += kLanes) in[d][q] = q < rows_here ? row[d] : 0u;
    }
    __syncthreads();
    stage_row(code, seq_rows(seq_tab), [&](int g) { return in[g][lane]; }, [&](int g, uint32_t word) { in[g][lane] = word; });
    TchIo io{ outw, dec_scratch + (size_t)blockIdx.x * dec_pairs * kLanes + lane, lane };
    const uint32_t biterr = decode_lane(ng, type2, biterr_out != nullptr, [&](int w) { return in[w][lane]; }, io);
    if (biterr_out && blk < n_blocks) biterr_out[blk] = biterr;
    __syncthreads();
    tch_write_rows(outw, lane, rows_here, type2, out + (size_t)blk0 * out_stride, out_stride);
}

// The TCH jobs of a soft frame launch: k_lmac_frames_soft's prologue and ring front end with the SCH/F layout, verdict 1 and the label;
// counts_tab.out[job] NULL: the job does not count.  The staged words lie [word][lane].
__global__ __launch_bounds__(kLanes) void k_tch_frames_soft(const JobTable tab, uint32_t* __restrict__ dec_scratch, const uint32_t* __restrict__ seq_tab,
                                                            const uint32_t* __restrict__ ring, uint32_t ring_words, const BiterrTable counts_tab) {
    using namespace tetra_tch_soft;
    __shared__ TchSoftCols in;
    __shared__ TchOutW outw;
    const int lane = threadIdx.x;
    FrameLane L = frame_group(tab, lane);
    if (L.blk0 >= L.n_blocks) return;
    frame_of(tab, L);
    const DevJob& J = L.J;
    frame_block(L.code, [&] { return tab.src.bitnum[L.f]; }, [&] { return tab.src.frame_type[L.f]; }, seq_rows(seq_tab),
                ring_of(ring, ring_words, L.f / tab.src.frames_per_channel), ring_words, [&](int g, uint32_t word) { in[g][lane] = word; });
    if (L.blk < L.n_blocks) write_verdict(J, tab.src, L.blk, L.f, true);
    TchIo io{ outw, dec_scratch + J.scratch_base + (size_t)L.group * J.dec_pairs * kLanes + lane, lane };
    uint32_t* counts = job_counts(tab, counts_tab);            // (workgroup-uniform: a workgroup has one job)
    const uint32_t biterr = decode_lane(tetra_tch::ng_of_type2(J.type2), J.type2, counts != nullptr, [&](int w) { return in[w][lane]; }, io);
    if (counts && L.blk < L.n_blocks) counts[L.blk] = biterr;
    __syncthreads();
    tch_write_rows(outw, lane, L.rows_here, J.type2, J.out + (size_t)L.blk0 * J.out_stride, J.out_stride);
}

// ---- the coded data channels interleaved over N = 1, 4 or 8 blocks (include/ext/tetra_tch_nblk.h; lane code: tch_nblk_core.hpp) --------------
// Kernels of their own behind a front end of their own; forward pass, traceback, counts, scratch [workgroup][step pair][lane] and row
// write-back are the siblings' above.  One wavefront per workgroup, an OUTPUT block per lane; ng and N are workgroup-uniform.
// How the rows reach the lanes: each lane gathers its own 432 positions from the pool, a byte a load.  The window table puts no bound
// on a workgroup's distinct rows (64 N of them, 221 KB at N = 8, when nothing slides), so staging rows through LDS would need a second
// route for tables that do not slide; a pre-pass that descrambles the pool once needs a pool-sized scratch and a second launch.  The
// (432, 103) permutation scatters every read by bytes whichever way the rows are held, and a sliding workgroup's 64 + N - 1 rows
// (30.7 KB) are read N times out of the vector cache and L2, not out of memory: the gather costs its 432 load instructions a lane, each
// touching 64 cache lines, not its bytes, at N = 1 as at N = 8, and much the same with 27 loads in flight as with 4
// (DESIGN.md 8.3 has the measurement and what staging the sliding case through LDS would cost).  A lane touches only its own column
// of every LDS array below.
// LDS per workgroup, k_tch_nblk: 3584 (one scrambling sequence a lane) + 7168 (the block as classes, then bits) + 2508 (decoded halves) =
// 13260 B, twelve workgroups per CU of 160 KB; k_tch_nblk_soft: 27648 (staged bytes) + 3584 (the sequence, and behind the gather the
// decoded halves in the same space) = 31232 B, five workgroups per CU as k_tch_rows_soft has.
struct NblkArgs {
    const void* pool;                  // [n_rows][in_stride] received bursts
    int n_rows, in_stride;
    const uint32_t* scramb_init;
    const int* init_index;             // of the pool's rows, or NULL
    const int* windows;                // [n_blocks][n]
    int n, n_blocks;
    const int* n_blocks_dev;
    int ng, type2;
    uint8_t* out;
    int out_stride;
    uint32_t* dec_scratch;
    int dec_pairs;
    const uint32_t* seq_tab;
    uint32_t* biterr_out;
};
// packed_ok = 0: every workgroup through the class route (tetra_lmac_debug_force_byte_route)
__global__ __launch_bounds__(kLanes) void k_tch_nblk(const NblkArgs a, int packed_ok) {
    using namespace tetra_tch_nblk;
    __shared__ uint32_t seq[kSeqWords][kLanes];
    __shared__ uint32_t cls[kClsWords + 1][kLanes];
    __shared__ TchOutW outw;
    const int lane = threadIdx.x;
    const int blk0 = blockIdx.x * kLanes;
    const int blk = blk0 + lane;
    int n_blocks = a.n_blocks;
    if (a.n_blocks_dev) {
        const int have = *a.n_blocks_dev;
        n_blocks = have < n_blocks ? have : n_blocks;
    }
    if (blk0 >= n_blocks) return;
    const int rows_here = min(kLanes, n_blocks - blk0);
    const bool live = blk < n_blocks;
    const uint8_t* pool = static_cast<const uint8_t*>(a.pool);
#pragma unroll
    for (int w = 0; w <= kClsWords; ++w) cls[w][lane] = 0u;
    // (a lane past the last block gathers nothing and does not speak for the route)
    const uint32_t dirty = gather_hard(live ? a.n : 0, a.n_rows, [&](int j) { return a.windows[(size_t)blk * a.n + j]; },
                                       [&](int r) { return a.scramb_init[a.init_index ? a.init_index[r] : r]; }, seq_rows(a.seq_tab),
                                       [&](int w, uint32_t word) { seq[w][lane] = word; }, [&](int w) { return seq[w][lane]; },
                                       [&](int r, int t) -> uint32_t { return pool[(size_t)r * a.in_stride + t]; },
                                       [&](int w, uint32_t bits) { cls[w][lane] |= bits; });
    const bool class_route = !packed_ok || __builtin_amdgcn_ballot_w64(dirty != 0) != 0;          // wave-uniform
    TchIo io{ outw, a.dec_scratch + (size_t)blockIdx.x * a.dec_pairs * kLanes + lane, lane };
    auto staged = [&](int w) { return cls[w][lane]; };
    uint32_t biterr;
    if (!class_route) {
        classes_to_bits(staged, [&](int w, uint32_t word) { cls[w][lane] = word; });
        biterr = tetra_tch::decode_lane<true>(a.ng, a.type2, a.biterr_out != nullptr, staged, io);
    } else {
        biterr = tetra_tch::decode_lane<false>(a.ng, a.type2, a.biterr_out != nullptr, staged, io);
    }
    if (a.biterr_out && live) a.biterr_out[blk] = biterr;
    __syncthreads();
    tch_write_rows(outw, lane, rows_here, a.type2, a.out + (size_t)blk0 * a.out_stride, a.out_stride);
}

__global__ __launch_bounds__(kLanes) void k_tch_nblk_soft(const NblkArgs a) {
    using namespace tetra_tch_nblk;
    __shared__ TchSoftCols in;
    __shared__ union { uint32_t seq[kSeqWords][kLanes]; TchOutW outw; } u;           // the sequence only while gathering
    static_assert(sizeof(TchOutW) <= sizeof(uint32_t) * kSeqWords * kLanes, "the decoded halves fit the sequence's space");
    const int lane = threadIdx.x;
    const int blk0 = blockIdx.x * kLanes;
    const int blk = blk0 + lane;
    int n_blocks = a.n_blocks;
    if (a.n_blocks_dev) {
        const int have = *a.n_blocks_dev;
        n_blocks = have < n_blocks ? have : n_blocks;
    }
    if (blk0 >= n_blocks) return;
    const int rows_here = min(kLanes, n_blocks - blk0);
    const bool live = blk < n_blocks;
    const uint8_t* pool = static_cast<const uint8_t*>(a.pool);
#pragma unroll
    for (int g = 0; g < kSoftWords; ++g) in[g][lane] = 0x80808080u;
    uint8_t* mine = reinterpret_cast<uint8_t*>(&in[0][lane]);
    gather_soft(live ? a.n : 0, a.n_rows, [&](int j) { return a.windows[(size_t)blk * a.n + j]; },
                [&](int r) { return a.scramb_init[a.init_index ? a.init_index[r] : r]; }, seq_rows(a.seq_tab),
                [&](int w, uint32_t word) { u.seq[w][lane] = word; }, [&](int w) { return u.seq[w][lane]; },
                [&](int r, int t) -> uint32_t { return pool[(size_t)r * a.in_stride + t]; },
                [&](int q, uint32_t y) { mine[(size_t)(q >> 2) * (4 * kLanes) + (q & 3)] = (uint8_t)y; });
    __syncthreads();                    // the sequence's space becomes the decoded halves'
    TchIo io{ u.outw, a.dec_scratch + (size_t)blockIdx.x * a.dec_pairs * kLanes + lane, lane };
    const uint32_t biterr = decode_lane(a.ng, a.type2, a.biterr_out != nullptr, [&](int w) { return in[w][lane]; }, io);
    if (a.biterr_out && live) a.biterr_out[blk] = biterr;
    __syncthreads();
    tch_write_rows(u.outw, lane, rows_here, a.type2, a.out + (size_t)blk0 * a.out_stride, a.out_stride);
}

// ---- list decoding of the rows whose CRC failed (include/ext/tetra_list.h; lane code: list_core.hpp) ------------------------------------------
// Four launches BEHIND a decode launch that was asked for ranks, on its stream, for ALL its jobs together, none otherwise.  The rows of
// the jobs with ranks form one index space, a job's rows rounded up to whole tiles of 256, so that a tile belongs to one job:
// k_list_count, k_list_scan and k_list_fill (compact_core.hpp's three steps over crc_ok == 0; the fill also writes every row's default
// rank, 0 for a good row and -1 for a failed one) leave ONE list of failed rows, job after job, and the scanned tile offsets say where
// a job's part of it begins.  k_list_rescue is a small persistent grid: a workgroup takes 64 failed rows of one job at a time, a row per
// lane, whichever workgroup decoded them, and strides over the list; with no failed row every workgroup reads a handful of words and
// leaves.  The cost is that of the failed rows.
// A lane stages its block again through the front end its decode launch used (FRONT: the same lmac_core.hpp / soft_core.hpp function), reads the decoder's decision words of its row
// from the launch's scratch -- which the host therefore hands back only behind this kernel --, and runs list_core.hpp's rescue.  The
// winner's row, verdict, label verdict, rank and (where the launch counts) channel bit errors are written by the lane itself: plain
// 4-byte stores to one row.
// Beside k_fused (compact_core.hpp's note): workgroups of 256 (compaction) and 64 threads.
constexpr int kListTile = 256;
constexpr int kRescueGroups = 512;         // the persistent grid (two per compute unit)
enum { kFrontBytes, kFrontFrames, kFrontSoft };
struct RescueJob {
    // the rows of a job of the decode launch
    const int* n_dev;
    int n;
    int first_tile;                    // of the launch's tiles, the job's first
    int* crc_ok;
    uint8_t* out;
    int out_stride;
    tetra_lmac_label_t* labels;
    uint32_t* counts;
    int32_t* rank;
    const uint32_t* dec;               // the rows' decision scratch, [workgroup][pair][lane]
    int dec_pairs;
    int type345, type2, a;
    // front ends: byte rows
    const uint8_t* type5;
    int in_stride, fixed_init;
    const uint32_t* scramb_init;
    const int* init_index;
    // ... frames and soft values
    const int* row_frame;
    const uint32_t* frame_scramb;
    int layout;
};
struct RescueTable {
    RescueJob job[TETRA_LMAC_MAX_JOBS];
    int n, tiles, T;
    // the compacted failed rows
    int* work;                         // [tiles]: failed rows per tile, scanned in place to the tile's first list position
    int* total;
    int* list;                         // [sum of the jobs' rows]: the failed rows' numbers within their job
    DevFrames src;
    const uint32_t* seq_tab;
    const uint32_t* ring;
    uint32_t ring_words;
};
__device__ __forceinline__ int list_rows(const RescueJob& J) {
    int n = J.n;
    if (J.n_dev) {
        const int have = *J.n_dev;
        n = have < n ? have : n;
    }
    return n;
}
__device__ __forceinline__ int job_of_tile(const RescueTable& tab, int tile) {
    int j = 0;
    for (int i = 1; i < tab.n; ++i) j = tile >= tab.job[i].first_tile ? i : j;
    return j;
}
__global__ __launch_bounds__(kListTile) void k_list_count(const RescueTable tab) {
    const int tile = (int)blockIdx.x;
    const RescueJob& J = tab.job[job_of_tile(tab, tile)];
    const int n = list_rows(J), t0 = (tile - J.first_tile) * kListTile;
    if (t0 >= n) {
        if (threadIdx.x == 0) tab.work[tile] = 0;
        return;
    }
    const int i = t0 + (int)threadIdx.x;
    compact_core::block_count<1>(i < n && J.crc_ok[i] == 0, tab.work, tab.tiles, tile);
}
__global__ __launch_bounds__(compact_core::kScanThreads) void k_list_scan(const RescueTable tab) {
    const int len[1] = { tab.tiles };
    compact_core::scan_counts<1>(tab.work, tab.tiles, len, tab.total);
}
__global__ __launch_bounds__(kListTile) void k_list_fill(const RescueTable tab) {
    const int tile = (int)blockIdx.x;
    const RescueJob& J = tab.job[job_of_tile(tab, tile)];
    const int n = list_rows(J), t0 = (tile - J.first_tile) * kListTile;
    if (t0 >= n) return;
    const int i = t0 + (int)threadIdx.x;
    const bool failed = i < n && J.crc_ok[i] == 0;
    int at[1];
    compact_core::block_rank<1, kListTile>(failed, at);
    if (failed) tab.list[tab.work[tile] + at[0]] = i;
    if (i < n) J.rank[i] = failed ? -1 : 0;
}
// LDS per workgroup: the staged block (byte rows 7168 B of soft classes, frames 3584 B of bits, soft values 27648 B) + 2376 (decoded
// halves) + 1024 (backward CRC table).  Every array but the table is a column per lane, so the rounds of the persistent loop need no
// barrier between them.
template <int FRONT>
__global__ __launch_bounds__(kLanes) void k_list_rescue(const RescueTable tab) {
    typedef uint32_t Staged[FRONT == kFrontSoft ? tetra_soft::kSoftWords : (FRONT == kFrontFrames ? kSeqWords : kClsWords + 1)][kLanes];
    __shared__ Staged in;
    __shared__ OutW outw;
    __shared__ uint32_t crc_inv[256];
    const int lane = threadIdx.x;
    const int total = *tab.total;
    if (total == 0) return;
    load_crc_inv(crc_inv, lane);
    __syncthreads();
    auto staged = [&](int w) { return in[w][lane]; };
    auto stage = [&](int w, uint32_t word) { in[w][lane] = word; };
    auto half = [&](int h) { return outw[h][lane]; };
    for (int v = (int)blockIdx.x;; v += (int)gridDim.x) {
        // group v of 64 failed rows, counted job after job (all of this is workgroup-uniform)
        int j = 0, u = v, first = 0, cnt = 0;
        for (; j < tab.n; ++j) {
            first = tab.work[tab.job[j].first_tile];
            cnt = (j + 1 < tab.n ? tab.work[tab.job[j + 1].first_tile] : total) - first;
            const int groups = (cnt + kLanes - 1) / kLanes;
            if (u < groups) break;
            u -= groups;
        }
        if (j >= tab.n) return;
        const RescueJob& a = tab.job[j];
        const int blk0 = u * kLanes;
        const bool live = blk0 + lane < cnt;
        const int row = tab.list[first + (live ? blk0 + lane : blk0)];     // (a lane without a row repeats the first one's work and writes nothing)
        LaneIo io{ outw, crc_inv, const_cast<uint32_t*>(a.dec) + (size_t)(row / kLanes) * a.dec_pairs * kLanes + row % kLanes, lane };
        int rank;
        uint32_t biterr = 0;
        if constexpr (FRONT == kFrontBytes) {
            // the byte route of k_lmac_decode, the lane reading its own row: classes of plain bits are the packed route's bits
            const uint32_t* rowp = reinterpret_cast<const uint32_t*>(a.type5 + (size_t)row * a.in_stride);
            byte_row_block(&a, a.fixed_init ? kScrambInitSb1 : a.scramb_init[a.init_index ? a.init_index[row] : row], [&](int d) { return rowp[d]; }, stage);
            rank = tetra_list::rescue_hard<false>(a.type345, a.type2, a.a, tab.T, staged, io, half);
            if (a.counts && rank > 0) biterr = bit_errors_hard<false>(a.type345, a.type2, a.a, half, staged);
        } else {
            const FrameRef fr = frame_lookup(a.row_frame[row], tab.src.n_frames, a.frame_scramb);
            const int f = fr.f;
            if constexpr (FRONT == kFrontFrames) {
                uint32_t fw[kFrameWords];
                load_frame(frame_rows(tab.src.frames, f), fw);
                frame_hard_block(&a, fr.code, fw, [&] { return tab.src.frame_type[f]; }, seq_rows(tab.seq_tab), stage);
                rank = tetra_list::rescue_hard<true>(a.type345, a.type2, a.a, tab.T, staged, io, half);
                if (a.counts && rank > 0) biterr = bit_errors_hard<true>(a.type345, a.type2, a.a, half, staged);
            } else {
                tetra_soft::soft_block(&a, fr.code, [&] { return tab.src.bitnum[f]; }, [&] { return tab.src.frame_type[f]; }, seq_rows(tab.seq_tab),
                                       ring_of(tab.ring, tab.ring_words, f / tab.src.frames_per_channel), tab.ring_words, stage);
                rank = tetra_list::rescue_soft(a.type345, a.type2, a.a, tab.T, staged, io, half);
                if (a.counts && rank > 0) biterr = tetra_soft::bit_errors_soft(a.type345, a.type2, a.a, half, staged);
            }
        }
        if (live) {
            a.rank[row] = rank;
            if (rank > 0) {
                uint32_t* dst = reinterpret_cast<uint32_t*>(a.out + (size_t)row * a.out_stride);
                for (int d = 0; d < a.type2 >> 2; ++d) dst[d] = spread4(((uint32_t)outw[d >> 2][lane] >> (4 * (d & 3))) & 0xfu);
                a.crc_ok[row] = 1;
                if (a.labels) a.labels[row].crc_ok = 1;
                if (a.counts) a.counts[row] = biterr;
            }
        }
    }
}

// One value per device, built on first use under a lock (safe for concurrent handles: one per GPU in a multi-GPU bank) and kept for the
// life of the process.  make(dev) returns the value, or a null one if it cannot be set up: get() then returns null, and tries again
// next time.
template <class T>
struct PerDevice {
    std::mutex mu;
    T v[64] = {};
    template <class Make>
    T get(Make make) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return T{};
        std::lock_guard<std::mutex> g(mu);
        if (!v[dev]) v[dev] = make(dev);
        return v[dev];
    }
};
// a table of `words` words filled on the host, on the current device (nullptr: out of memory, the caller reports TETRA_ERR_NOMEM)
uint32_t* upload_table(size_t words, void (*fill)(uint32_t*)) {
    std::vector<uint32_t> host(words);
    fill(host.data());
    DevMem<uint32_t> d_tab;
    if (d_tab.reserve(sizeof(uint32_t) * words) != hipSuccess || hipMemcpy(d_tab, host.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return d_tab.release();
}
// the packed route's scrambling-sequence table (64 KB)
const uint32_t* seq_table() {
    static PerDevice<uint32_t*> tab;
    return tab.get([](int) { return upload_table((size_t)4 * 256 * kSeqStride, scramb_sequence_table); });
}
// the AACH's Reed-Muller decoding (tetra_aach.h): syndrome -> error pattern, 2^16 entries = 256 KB, from the generator
const uint32_t* rm3014_table() {
    static PerDevice<uint32_t*> tab;
    return tab.get([](int) { return upload_table(kRm3014TableEntries, rm3014_correction_table); });
}

// The decoder's decision scratch (up to 200 MB for a second of 4096 channels' SCH/F slots) comes from a stream-ordered pool of this
// library's own, one per device, that KEEPS what is freed into it (release threshold = everything).  The device's default pool hands
// unused memory back to the driver at synchronisation points; the next call then maps 200 MB again and takes milliseconds instead of
// microseconds -- seen as one call in five at 20 ms in the two-stream chain (profiles/r05/README.md).
hipMemPool_t scratch_pool() {
    static PerDevice<hipMemPool_t> pool;
    return pool.get([](int dev) -> hipMemPool_t {
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t p = nullptr;
        if (hipMemPoolCreate(&p, &props) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        uint64_t keep = ~0ull;
        (void)hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &keep);
        return p;
    });
}
// One launch's lease of decision scratch: the caller's workspace if it gave one, else `bytes` from the keeping pool (after the first
// call a free-list hit; the device's default pool if the keeping pool could not be made), handed back in stream order right behind
// the kernel.
struct ScratchLease {
    uint32_t* p = nullptr;
    hipStream_t s = nullptr;
    bool pooled = false;
    int take(size_t bytes, void* workspace, size_t workspace_bytes, hipStream_t stream) {
        s = stream;
        if (workspace) {
            if (workspace_bytes < bytes) return TETRA_ERR_SIZE;
            if ((uintptr_t)workspace & 3) return TETRA_ERR_ALIGN;
            p = static_cast<uint32_t*>(workspace);
            return TETRA_OK;
        }
        hipMemPool_t pool = scratch_pool();
        const hipError_t got = pool ? hipMallocFromPoolAsync(reinterpret_cast<void**>(&p), bytes, pool, s) : hipMallocAsync(reinterpret_cast<void**>(&p), bytes, s);
        if (got != hipSuccess) { (void)hipGetLastError(); return TETRA_ERR_NOMEM; }
        pooled = true;
        return TETRA_OK;
    }
    bool give_back() { return !pooled || hipFreeAsync(p, s) == hipSuccess; }
    // behind the launch: its status and the hand-back's
    int launched() {
        const hipError_t launch = hipGetLastError();
        return !give_back() || launch != hipSuccess ? TETRA_ERR_HIP : TETRA_OK;
    }
};

// The list launches behind a decode launch on stream s.  tab: the jobs with ranks (n of them, everything but first_tile) and what they
// share; the compaction's own words come from the caller's workspace `ws` if it gave one (the chain's handle), else from the keeping pool,
// handed back in stream order behind the rescue kernel.
size_t list_words(long long tiles, long long rows) { return (size_t)tiles + 1 + (size_t)rows; }
int launch_list(int front, RescueTable& tab, hipStream_t s, void* ws, size_t ws_bytes) {
    long long tiles = 0, rows = 0, groups = 0;
    for (int k = 0; k < tab.n; ++k) {
        tab.job[k].first_tile = (int)tiles;
        tiles += (tab.job[k].n + kListTile - 1) / kListTile;
        rows += tab.job[k].n;
        groups += (tab.job[k].n + kLanes - 1) / kLanes;
    }
    if (tab.n == 0) return TETRA_OK;
    if (tiles > 0x7fffffffLL) return TETRA_ERR_SIZE;
    tab.tiles = (int)tiles;
    ScratchLease w;
    if (const int err = w.take(sizeof(int) * list_words(tiles, rows), ws, ws_bytes, s)) return err;
    tab.work = reinterpret_cast<int*>(w.p);
    tab.total = tab.work + tab.tiles;
    tab.list = tab.total + 1;
    const dim3 grid((unsigned)(groups < kRescueGroups ? groups : kRescueGroups));
    hipLaunchKernelGGL(k_list_count, dim3(tab.tiles), dim3(kListTile), 0, s, tab);
    hipLaunchKernelGGL(k_list_scan, dim3(1), dim3(compact_core::kScanThreads), 0, s, tab);
    hipLaunchKernelGGL(k_list_fill, dim3(tab.tiles), dim3(kListTile), 0, s, tab);
    if (front == kFrontBytes) hipLaunchKernelGGL(k_list_rescue<kFrontBytes>, grid, dim3(kLanes), 0, s, tab);
    else if (front == kFrontFrames) hipLaunchKernelGGL(k_list_rescue<kFrontFrames>, grid, dim3(kLanes), 0, s, tab);
    else hipLaunchKernelGGL(k_list_rescue<kFrontSoft>, grid, dim3(kLanes), 0, s, tab);
    return w.launched();
}
// The next job of a rescue table, what every front end's job holds filled in: the rows, where their results go, their decision scratch and
// their kind.  The caller adds its front end's own fields.
RescueJob& add_rescue_job(RescueTable& rt, const int* n_dev, int n, int* crc_ok, uint8_t* out, int out_stride, tetra_lmac_label_t* labels, uint32_t* counts,
                          int32_t* rank, const uint32_t* dec, int dec_pairs, int type345, int type2, int a) {
    RescueJob& j = rt.job[rt.n++];
    j.n_dev = n_dev; j.n = n; j.crc_ok = crc_ok; j.out = out; j.out_stride = out_stride; j.labels = labels; j.counts = counts; j.rank = rank;
    j.dec = dec; j.dec_pairs = dec_pairs; j.type345 = type345; j.type2 = type2; j.a = a;
    return j;
}
// a rank array and its T (tetra_list.h): none, or a 4-byte aligned array with T in 1..8
int check_list(const void* d_rank, int max_candidates) {
    if (!d_rank) return TETRA_OK;
    if (max_candidates < 1 || max_candidates > tetra_list::kMaxCandidates) return TETRA_ERR_ARG;
    return ((uintptr_t)d_rank & 3) ? TETRA_ERR_ALIGN : TETRA_OK;
}

// TPSAP_T_BBK: the reference only descrambles (tetra_lower_mac.c:231-236); 30 bits per block, one lane per block.
// RM (tetra_lmac_decode_aach_rm3014_device): the descrambled bytes are also gathered into the 30-bit word (a byte other than 0 is a 1),
// rm3014_decode runs on it, a decodable row is rewritten with the codeword's bits, byte 30 takes the distance and byte 31 a zero
// (rows of at least 32 bytes).  The table is a trailing parameter pack -- one pointer for RM, none otherwise -- so that the instantiation
// without the option has the argument block, and with it the instruction stream, it had before the option existed.
template <bool RM, class... Tab>
__global__ __launch_bounds__(256) void k_lmac_bbk(const uint8_t* __restrict__ type5, int n_blocks, int in_stride,
                                                  const uint32_t* __restrict__ scramb_init, int nbits,
                                                  uint8_t* __restrict__ out, int out_stride, int* __restrict__ crc_ok,
                                                  const int* __restrict__ n_blocks_dev, const int* __restrict__ init_index,
                                                  Tab... rm_tab_pack) {
    const int blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (blk >= n_blocks || (n_blocks_dev && blk >= *n_blocks_dev)) return;
    uint32_t lfsr = scramb_init[init_index ? init_index[blk] : blk];
    const uint8_t* src = type5 + (size_t)blk * in_stride;
    uint8_t* dst = out + (size_t)blk * out_stride;
    if constexpr (!RM) {
        for (int j = 0; j < nbits; ++j) dst[j] = src[j] ^ (uint8_t)lfsr_next(lfsr);
        crc_ok[blk] = 1;
    } else {
        const uint32_t* __restrict__ rm_tab = only_of(rm_tab_pack...);
        uint32_t word = 0;
        for (int j = 0; j < 30; ++j) {
            const uint8_t v = src[j] ^ (uint8_t)lfsr_next(lfsr);
            dst[j] = v;
            word = (word << 1) | (v ? 1u : 0u);
        }
        const Rm3014Word r = rm3014_decode(word, [&](uint32_t s) { return rm_tab[s]; });
        const bool good = r.dist <= (uint32_t)kRm3014Radius;
        if (good)
            for (int j = 0; j < 30; ++j) dst[j] = (uint8_t)((r.word >> (29 - j)) & 1u);
        dst[30] = (uint8_t)r.dist;
        dst[31] = 0;
        crc_ok[blk] = good;
    }
}

// the bare primitive (tetra_lmac_rm3014_decode_device): a lane per 30-bit word
__global__ __launch_bounds__(256) void k_rm3014(const uint32_t* __restrict__ words, int n, uint32_t* __restrict__ out_words,
                                                uint8_t* __restrict__ dist, const uint32_t* __restrict__ rm_tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Rm3014Word r = rm3014_decode(words[i], [&](uint32_t s) { return rm_tab[s]; });
    out_words[i] = r.word;
    dist[i] = (uint8_t)r.dist;
}

// ---- the AACH from soft values: exact maximum-likelihood decoding (include/ext/tetra_aach_soft.h; lane code: soft_core.hpp) --------------
// corr[codeword][block] = sum over k of (+-1)[codeword][k] * y[k][block] is a 16384 x 32 (30 padded) by 32 x blocks integer product:
// v_mfma_i32_32x32x32_i8, a wavefront per 32 blocks, 512 steps of 32 codewords each.  Operand A holds the codewords (a row of the result
// = a codeword of the step), operand B the blocks (a column = a block), so a lane's 16 result registers are 16 codewords of ONE block,
// its own (column = lane & 31; rows (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), and the running best two need no lane crossing until the
// end, where the two lanes of a block merge.  Both operands give lane (r, h = lane >> 5) element j the same k = 16 h + j of their row r,
// so the products pair up whichever k the hardware gives that element.
// The +-1 matrix is never in memory.  The code is linear: codeword(32 t + r) = codeword(32 t) ^ codeword(r), and in bytes of +-1 (0x01 /
// 0xff) a flipped sign is an XOR with 0xfe.  A lane keeps the 16 bytes of codeword(r) and XORs step t's 16 flip bytes of its half onto
// them: `flip` [512][2] x 16 B = 16 KB of LDS, which the workgroup fills from the generator on entry.
// Per product the epilogue is three vector instructions: key = corr << 14 + 32 (511 - t) (the step's share of 16383 - info, a scalar),
// second = med3(best, second, key), best = max(best, key), one (best, second) pair per result register; the row's share of the key, 31 - row, is
// added once behind the loop.  The next step's MFMA is issued in front of a step's epilogue.
// A workgroup is four wavefronts = 128 blocks sharing the flip table: 16 KB of LDS and four wave slots, which is what k_fused leaves on a
// compute unit.
typedef int AachV4 __attribute__((ext_vector_type(4)));
typedef int AachV16 __attribute__((ext_vector_type(16)));
constexpr int kAachWaveRows = 32;
constexpr int kAachGroupThreads = 256;
constexpr int kAachGroupRows = kAachWaveRows * kAachGroupThreads / kLanes;          // 128: the kernel's row tile
constexpr int kAachSteps = 16384 / 32;
typedef uint4 AachFlip[kAachSteps][2];

// the +-1 bytes' flip masks of a codeword's bits 16 h .. 16 h + 15 (cw: first bit on air at bit 31); bits 30, 31 are no part of it
__device__ __forceinline__ uint4 aach_flip_bytes(uint32_t cw, int h) {
    const uint32_t half = (cw << (16 * h)) >> 16;
    return uint4{ tetra_soft::nibble_mask((half >> 12) & 0xfu) & 0xfefefefeu, tetra_soft::nibble_mask((half >> 8) & 0xfu) & 0xfefefefeu,
                  tetra_soft::nibble_mask((half >> 4) & 0xfu) & 0xfefefefeu, tetra_soft::nibble_mask(half & 0xfu) & 0xfefefefeu };
}
__device__ __forceinline__ void aach_fill_flip(AachFlip& flip) {
    for (int e = (int)threadIdx.x; e < 2 * kAachSteps; e += kAachGroupThreads)
        flip[e >> 1][e & 1] = aach_flip_bytes(rm3014_encode(32u * (uint32_t)(e >> 1)) << 2, e & 1);
}
__device__ __forceinline__ AachV16 aach_step(const uint4& a0, const uint4& m, const AachV4& b) {
    const AachV4 a = { (int)(a0.x ^ m.x), (int)(a0.y ^ m.y), (int)(a0.z ^ m.z), (int)(a0.w ^ m.w) };
    const AachV16 zero = {};
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, zero, 0, 0, 0);
}
// the best two keys (soft_core.hpp aach_key) of the lane's block, lane & 31 of the wavefront's 32, over all codewords; y: its staged row
__device__ __forceinline__ tetra_soft::Top2 aach_search(const uint32_t y[tetra_soft::kAachWords], const AachFlip& flip) {
    using namespace tetra_soft;
    const int lane = (int)threadIdx.x & (kLanes - 1), h = lane >> 5;
    const uint4 f0 = aach_flip_bytes(rm3014_encode((uint32_t)(lane & 31)) << 2, h);
    const uint4 a0 = { f0.x ^ 0x01010101u, f0.y ^ 0x01010101u, f0.z ^ 0x01010101u, f0.w ^ 0x01010101u };
    const AachV4 b = { (int)y[4 * h], (int)y[4 * h + 1], (int)y[4 * h + 2], (int)y[4 * h + 3] };
    Top2 slot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) slot[r] = Top2{ kTop2None, kTop2None };
    AachV16 acc = aach_step(a0, flip[0][h], b);
#pragma unroll 2
    for (int t = 0; t < kAachSteps; ++t) {
        const AachV16 next = aach_step(a0, flip[t + 1 < kAachSteps ? t + 1 : t][h], b);       // (the last one is not used)
        const int step_key = 32 * (kAachSteps - 1 - t);
#pragma unroll
        for (int r = 0; r < 16; ++r) top2_insert(slot[r], (int)(((uint32_t)acc[r] << 14) + (uint32_t)step_key));
        acc = next;
    }
    Top2 top{ kTop2None, kTop2None };
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row_key = 31 - ((r & 3) + 8 * (r >> 2) + 4 * h);
        top2_insert(top, slot[r].best + row_key);
        top2_insert(top, slot[r].second + row_key);          // (same register: same row)
    }
    const int ob = __shfl_xor(top.best, 32), os = __shfl_xor(top.second, 32);
    top2_insert(top, ob);
    top2_insert(top, os);
    return top;
}

// the bare primitive (tetra_lmac_rm3014_soft_decode_device)
__global__ __launch_bounds__(kAachGroupThreads) void k_aach_soft(const int8_t* __restrict__ soft, int n, int soft_stride, uint32_t* __restrict__ out_words,
                                                                 uint8_t* __restrict__ dist, uint16_t* __restrict__ margin) {
    using namespace tetra_soft;
    __shared__ AachFlip flip;
    aach_fill_flip(flip);
    __syncthreads();
    const int lane = (int)threadIdx.x & (kLanes - 1);
    const int blk0 = ((int)blockIdx.x * (kAachGroupThreads / kLanes) + (int)threadIdx.x / kLanes) * kAachWaveRows;
    if (blk0 >= n) return;
    const int blk = blk0 + (lane & 31);
    uint32_t y[kAachWords];
    const uint32_t* row = reinterpret_cast<const uint32_t*>(soft + (size_t)(blk < n ? blk : blk0) * soft_stride);
#pragma unroll
    for (int g = 0; g < kAachWords; ++g) y[g] = row[g];
    y[kAachWords - 1] &= 0x0000ffffu;
    const Top2 top = aach_search(y, flip);
    if (lane < kAachWaveRows && blk < n) {
        const AachSoft r = aach_soft_finish(top, y);
        if (out_words) out_words[blk] = r.word;
        if (dist) dist[blk] = (uint8_t)r.dist;
        if (margin) margin[blk] = (uint16_t)r.margin;
    }
}

// a soft BBK job of the frame decoder (TETRA_LMAC_JOB_RM3014_SOFT): the staging of soft_core.hpp's aach_soft_block in front of the search,
// rows, verdicts and labels behind it as k_lmac_frames writes a BBK job's
__global__ __launch_bounds__(kAachGroupThreads) void k_aach_soft_frames(const DevJob J, const DevFrames src, const uint32_t* __restrict__ seq_tab,
                                                                        const uint32_t* __restrict__ ring, uint32_t ring_words, int min_margin) {
    using namespace tetra_soft;
    __shared__ AachFlip flip;
    aach_fill_flip(flip);
    __syncthreads();
    const int lane = (int)threadIdx.x & (kLanes - 1);
    const int blk0 = ((int)blockIdx.x * (kAachGroupThreads / kLanes) + (int)threadIdx.x / kLanes) * kAachWaveRows;
    int n = J.n_rows;
    if (J.n_rows_dev) {
        const int have = *J.n_rows_dev;
        n = have < n ? have : n;
    }
    if (blk0 >= n) return;
    const int blk = blk0 + (lane & 31);
    const FrameRef fr = frame_lookup(J.row_frame[blk < n ? blk : blk0], src.n_frames, J.frame_scramb);
    uint32_t y[kAachWords];
    aach_soft_block(fr.code, [&] { return src.bitnum[fr.f]; }, [&] { return src.frame_type[fr.f]; }, seq_rows(seq_tab),
                    ring_of(ring, ring_words, fr.f / src.frames_per_channel), ring_words, y);
    const Top2 top = aach_search(y, flip);
    if (lane < kAachWaveRows && blk < n) {
        const AachSoft r = aach_soft_finish(top, y);
        const uint32_t bits = r.word << 2, tail = aach_soft_tail(r);
        demux_core::U2* dst = reinterpret_cast<demux_core::U2*>(J.out + (size_t)blk * J.out_stride);
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = demux_core::U2{ bbk_bytes(bits, 2 * k), bbk_bytes(bits, 2 * k + 1) | (k == 3 ? tail : 0u) };
        write_verdict(J, src, blk, fr.f, aach_soft_good(r, min_margin));
    }
}

// The SB1 tracking rule, every entry point's: the SYNC-PDU read-out of tp_sap_udata_ind's SB1 case (tetra_lower_mac.c:246-275, with the
// copy of the PHY time into tcd->time at :172) plus the PHY's TDMA clock (tetra_burst_sync.c:113, tetra_tdma.c:28-78), per channel,
// frame slots in time order:
//   every frame the LOCKED receiver consumes      t_phy_state.time += one timeslot (tetra_tdma_time_add_tn, before the callback)
//   a SYNC burst's SB1 block, good CRC            tcd-> colour code, mcc, mnc, scramb_init; tcd->time (tn = bits + 1, fn, mn) -> t_phy_state.time
//   a SYNC burst's SB1 block, bad CRC             t_phy_state.time stays at its time on entry (tcd->time IS that time since :172, and
//                                                 :268 copies it back unchanged)
// Outputs per frame slot: the scrambling code in force for the slot's other blocks, the TDMA time tetra_burst_rx_cb sees on
// entry (t_display_st->curr_multiframe / curr_frame, tetra_burst.c:349-350) and the time after the slot's SB1 (what every
// later block of the burst and the next slot's increment start from).  Times are packed tn | fn << 8 | mn << 16 (tdma_pack).
//
// No walk over the slots: one wavefront per channel, 64 frame slots at a time, a slot per lane.  What a slot needs from its past is
// the last SYNC frame with a GOOD CRC before it -- the PHY clock was set to the PDU's time there, and tcd holds its fields -- and how
// many slots ago that was: "highest set bit below my lane" of the ballot of good frames; the fields travel with lane shuffles; and the
// clock k slots after it was set is tdma_advance.  Nothing is serial but the carry from one 64-slot group to the next.  The rule itself
// (track_slot, track_carry) lives in lmac_core.hpp, where the host emulation runs it too.  (A walk on the scalar unit: 2577 scalar
// instructions per wave, 29 us.)
//
// Two compile-time choices:
//   ROWS   kRowsList: the SB1 rows are compact, one per SYNC-list entry (tetra_lmac_track_sync_lists_device): a slot holds a SYNC
//                     burst where `present` (the frame types) says TETRA_TRAIN_SYNC, its row is chan_first[c] + the channel's SYNC
//                     slots before it, read as words (4-byte aligned rows);
//          kRowsSlot: one row per frame slot (tetra_lmac_track_sync_device / _scramb_device): the row of slot r is r, a slot holds
//                     one where `present` (d_valid) is non-zero, read as bytes (any stride, any row alignment)
//   State  tetra_lmac_cell_state_t (both times, labels) or uint32_t (tetra_lmac_track_scramb_device: the code alone, every slot live)
enum { kRowsList, kRowsSlot };
static_assert(sizeof(TrackState) == sizeof(tetra_lmac_cell_state_t), "TrackState is tetra_lmac_cell_state_t member for member");
__device__ __forceinline__ TrackState load_state(const tetra_lmac_cell_state_t& s) {
    return TrackState{ s.scramb_init, s.colour_code, s.mcc, s.mnc, Tdma{ s.tcd_tn, s.tcd_fn, s.tcd_mn }, Tdma{ s.phy_tn, s.phy_fn, s.phy_mn } };
}
__device__ __forceinline__ TrackState load_state(uint32_t code) {
    TrackState s = {};
    s.scramb_init = code;
    return s;
}
__device__ __forceinline__ void store_state(tetra_lmac_cell_state_t& d, const TrackState& s) {
    d = tetra_lmac_cell_state_t{ s.scramb_init, s.colour, s.mcc, s.mnc, s.tcd.tn, s.tcd.fn, s.tcd.mn, s.phy.tn, s.phy.fn, s.phy.mn };
}
__device__ __forceinline__ void store_state(uint32_t& d, const TrackState& s) { d = s.scramb_init; }
__device__ __forceinline__ uint32_t shfl_u32(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src); }
__device__ __forceinline__ Tdma shfl_tdma(const Tdma& t, int src) { return Tdma{ shfl_u32(t.tn, src), shfl_u32(t.fn, src), shfl_u32(t.mn, src) }; }
template <int ROWS, class State>
__global__ __launch_bounds__(kLanes) void k_track(const uint8_t* __restrict__ sb1, int stride, const int* __restrict__ crc_ok,
                                                  const int* __restrict__ present, const int* __restrict__ n_frames,
                                                  const int* __restrict__ chan_first, int frames, State* __restrict__ state,
                                                  uint32_t* __restrict__ row_scramb, uint32_t* __restrict__ row_time_rx,
                                                  uint32_t* __restrict__ row_time, const uint32_t* __restrict__ frame_bitnum,
                                                  tetra_lmac_label_t* __restrict__ labels) {
    using Row = typename std::conditional<ROWS == kRowsList, int, size_t>::type;      // a list position, or the slot
    const int c = blockIdx.x, lane = threadIdx.x;
    const int nf = n_frames ? min(n_frames[c], frames) : frames;
    int base = ROWS == kRowsList ? chan_first[c] : 0;
    TrackState st = load_state(state[c]);    // wave-uniform; carried from group to group
    for (int f0 = 0; f0 < frames; f0 += kLanes) {
        const int f = f0 + lane;
        const size_t r = (size_t)c * frames + f;
        const bool is_sync = f < frames && (ROWS == kRowsList ? present[r] == TETRA_TRAIN_SYNC : present[r] != 0);
        const unsigned long long m = __ballot(is_sync);
        const Row j = ROWS == kRowsList ? (Row)(base + __popcll(m & ((1ull << lane) - 1ull))) : (Row)r;      // the slot's SB1 row
        base += __popcll(m);
        // a, b: the PDU words of a SYNC frame with a good CRC (sync_pdu_words)
        const bool valid = is_sync && f < nf;
        bool good = false;
        uint32_t a = 0, b = 0;
        if (valid && crc_ok[j]) {
            good = true;
            const uint8_t* t2 = sb1 + (size_t)j * stride;
            sync_pdu_words([&](int k) -> uint32_t {              // bytes 4k .. 4k+3 of the row, little endian
                if (ROWS == kRowsList) return reinterpret_cast<const uint32_t*>(t2)[k];
                return t2[4 * k] | (t2[4 * k + 1] << 8) | (t2[4 * k + 2] << 16) | ((uint32_t)t2[4 * k + 3] << 24);
            }, a, b);
        }
        const unsigned long long mv = __ballot(valid), mg = __ballot(good);
        // the rule (every lane: a shuffle reads active lanes only)
        const TrackSlot me = track_slot(st, mv, mg, lane, [&](int h, uint32_t& ah, uint32_t& bh) { ah = shfl_u32(a, h); bh = shfl_u32(b, h); });
        const bool live = f < nf;
        // the group's last live slot is the state the next group (and the next call) starts from; slots past the channel's frame
        // count carry the code in force at its end
        const int last_live = min(nf - f0, kLanes) - 1;                       // < 0: no live slot in this group
        const int src = last_live < 0 ? 0 : last_live;
        const TrackSlot end = { shfl_tdma(me.t_rx, src), shfl_tdma(me.t_after, src), shfl_tdma(me.tcd, src),
                                shfl_u32(me.colour, src), shfl_u32(me.mcc, src), shfl_u32(me.mnc, src), shfl_u32(me.scramb, src) };
        const uint32_t code_end = last_live < 0 ? st.scramb_init : end.scramb;
        if (f < frames) {
            const uint32_t o_rx = live ? tdma_pack(me.t_rx) : 0u, o_t = live ? tdma_pack(me.t_after) : 0u;
            row_scramb[r] = live ? me.scramb : code_end;
            if (row_time_rx) row_time_rx[r] = o_rx;
            if (row_time) row_time[r] = o_t;
            if (labels && valid) {
                tetra_lmac_label_t lb;
                lb.channel = c;
                lb.frame_slot = f;
                lb.bitnum = frame_bitnum[r];
                lb.tdma_time_rx = o_rx;
                lb.tdma_time = o_t;
                lb.crc_ok = good;
                labels[j] = lb;
            }
        }
        if (last_live >= 0) track_carry(st, end);
    }
    if (lane == 0) store_state(state[c], st);
}

int check_args(int type, const void* in, int n_blocks, int in_stride, const void* init, const void* out, int out_stride,
               const void* ok, bool device_ptrs) {
    if (type < 0 || type > 5 || n_blocks < 0) return TETRA_ERR_ARG;
    if (n_blocks == 0) return TETRA_OK;
    if (!in || !out || !ok) return TETRA_ERR_ARG;
    if (type != TETRA_TPSAP_T_SB1 && !init) return TETRA_ERR_ARG;
    const BlkParam& p = blk_param(type);
    if (in_stride < p.type345 || out_stride < p.type2) return TETRA_ERR_ARG;
    if ((in_stride & 3) || (out_stride & 3)) return TETRA_ERR_ALIGN;
    if (device_ptrs && (((uintptr_t)in & 3) || ((uintptr_t)out & 3))) return TETRA_ERR_ALIGN;
    return TETRA_OK;
}

}  // namespace

extern "C" {

int tetra_lmac_blk_param(int type, tetra_lmac_blk_param_t* out) {
    if (type < 0 || type > 5 || !out) return TETRA_ERR_ARG;
    const BlkParam& p = blk_param(type);
    out->type345_bits = p.type345;
    out->type2_bits = p.type2;
    out->type1_bits = p.type1;
    out->interleave_a = p.a;
    out->have_crc16 = p.crc;
    return TETRA_OK;
}

uint32_t tetra_lmac_scramb_init(uint16_t mcc, uint16_t mnc, uint8_t colour) { return scramb_code(colour, mcc, mnc); }

int tetra_lmac_decode_batch_device(int type, const uint8_t* d_type5, int n_blocks, int in_stride, const uint32_t* d_scramb_init,
                                   uint8_t* d_type2, int out_stride, int32_t* d_crc_ok, void* hip_stream) {
    return tetra_lmac_decode_counted_device(type, d_type5, n_blocks, nullptr, in_stride, d_scramb_init, nullptr, d_type2, out_stride,
                                            d_crc_ok, hip_stream);
}

int tetra_lmac_decode_counted_device(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                     const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                     int32_t* d_crc_ok, void* hip_stream) {
    return tetra_lmac_decode_counted_biterr_device(type, d_type5, n_blocks, d_n_blocks, in_stride, d_scramb_init, d_init_index, d_type2, out_stride,
                                                   d_crc_ok, nullptr, hip_stream);
}

static int decode_counted(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                          const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                          int32_t* d_crc_ok, uint32_t* d_biterr, int max_candidates, int32_t* d_rank, void* hip_stream);

int tetra_lmac_decode_counted_biterr_device(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                            const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                            int32_t* d_crc_ok, uint32_t* d_biterr, void* hip_stream) {
    return decode_counted(type, d_type5, n_blocks, d_n_blocks, in_stride, d_scramb_init, d_init_index, d_type2, out_stride, d_crc_ok, d_biterr, 0, nullptr,
                          hip_stream);
}

int tetra_lmac_decode_counted_list_device(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                          const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                          int32_t* d_crc_ok, int max_candidates, int32_t* d_rank, void* hip_stream) {
    return decode_counted(type, d_type5, n_blocks, d_n_blocks, in_stride, d_scramb_init, d_init_index, d_type2, out_stride, d_crc_ok, nullptr,
                          max_candidates, d_rank, hip_stream);
}

// every byte-row entry point; d_rank NULL: the launches they always made, nothing else
static int decode_counted(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                          const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                          int32_t* d_crc_ok, uint32_t* d_biterr, int max_candidates, int32_t* d_rank, void* hip_stream) {
    if (d_rank && type == TETRA_TPSAP_T_BBK) return TETRA_ERR_ARG;              // the AACH has no CRC to aim at
    if (const int bad = check_list(d_rank, max_candidates)) return bad;
    const int rc = check_args(type, d_type5, n_blocks, in_stride, d_scramb_init, d_type2, out_stride, d_crc_ok, true);
    if (rc != TETRA_OK) return rc;
    if (d_biterr && type == TETRA_TPSAP_T_BBK) return TETRA_ERR_ARG;           // the AACH is not convolutionally coded: tetra_aach.h has its distance
    if ((uintptr_t)d_biterr & 3) return TETRA_ERR_ALIGN;
    if (n_blocks == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const BlkParam& p = blk_param(type);
    if (type == TETRA_TPSAP_T_BBK) {
        hipLaunchKernelGGL(k_lmac_bbk<false>, dim3((n_blocks + 255) / 256), dim3(256), 0, s, d_type5, n_blocks, in_stride, d_scramb_init,
                           p.type345, d_type2, out_stride, d_crc_ok, d_n_blocks, d_init_index);
    } else {
        // decision scratch: (type2 + 4) steps x 64 lanes x u16 per workgroup
        const int groups = (n_blocks + kLanes - 1) / kLanes;
        const int dec_pairs = (p.type2 + kFlush) / 2;
        const size_t bytes = (size_t)groups * dec_pairs * kLanes * sizeof(uint32_t);
        const uint32_t* seq = seq_table();
        if (!seq) return TETRA_ERR_NOMEM;
        ScratchLease scratch;
        if (const int err = scratch.take(bytes, nullptr, 0, s)) return err;
        const uint32_t* seq_or_bytes = g_force_byte_route ? nullptr : seq;
        if (d_biterr)
            hipLaunchKernelGGL((k_lmac_decode<true, uint32_t*>), dim3(groups), dim3(kLanes), 0, s, d_type5, n_blocks, in_stride, d_scramb_init,
                               type == TETRA_TPSAP_T_SB1 ? 1 : 0, p.type345, p.type2, p.type1, p.a, d_type2, out_stride, d_crc_ok,
                               scratch.p, dec_pairs, d_n_blocks, d_init_index, seq_or_bytes, d_biterr);
        else
            hipLaunchKernelGGL(k_lmac_decode<false>, dim3(groups), dim3(kLanes), 0, s, d_type5, n_blocks, in_stride, d_scramb_init,
                               type == TETRA_TPSAP_T_SB1 ? 1 : 0, p.type345, p.type2, p.type1, p.a, d_type2, out_stride, d_crc_ok,
                               scratch.p, dec_pairs, d_n_blocks, d_init_index, seq_or_bytes);
        int list_rc = TETRA_OK;
        if (d_rank) {               // behind the decode launch, in front of the scratch's hand-back
            RescueTable rt = {};
            RescueJob& a = add_rescue_job(rt, d_n_blocks, n_blocks, d_crc_ok, d_type2, out_stride, nullptr, d_biterr, d_rank, scratch.p, dec_pairs, p.type345, p.type2, p.a);
            a.type5 = d_type5; a.in_stride = in_stride; a.fixed_init = type == TETRA_TPSAP_T_SB1 ? 1 : 0; a.scramb_init = d_scramb_init; a.init_index = d_init_index;
            rt.T = max_candidates;
            list_rc = launch_list(kFrontBytes, rt, s, nullptr, 0);
        }
        const int launch_rc = scratch.launched();
        return list_rc != TETRA_OK ? list_rc : launch_rc;
    }
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

// ---- include/ext/tetra_tch.h: byte rows ----------------------------------------------------------------------------------------------
int tetra_lmac_tch_blk_param(int kind, tetra_lmac_blk_param_t* out) {
    if (!tetra_tch::is_tch(kind) || !out) return TETRA_ERR_ARG;
    const tetra_tch::Kind k = tetra_tch::kind_of(kind);
    out->type345_bits = tetra_tch::kType345;
    out->type2_bits = k.type2;
    out->type1_bits = k.type1;
    out->interleave_a = k.ng ? tetra_tch::kInterleaveA : 0;
    out->have_crc16 = 0;
    return TETRA_OK;
}

// check_args for a TCH kind (no verdicts; counts only for the coded kinds)
static int tch_check_args(int kind, const void* in, int n_blocks, int in_stride, const void* init, const void* out, int out_stride,
                          const void* biterr, bool device_ptrs) {
    if (!tetra_tch::is_tch(kind) || n_blocks < 0) return TETRA_ERR_ARG;
    if (biterr && kind == TETRA_LMAC_T_TCH_7_2) return TETRA_ERR_ARG;           // not coded: nothing to encode again
    if (n_blocks == 0) return TETRA_OK;
    if (!in || !out || !init) return TETRA_ERR_ARG;
    if (in_stride < tetra_tch::kType345 || out_stride < tetra_tch::kind_of(kind).type2) return TETRA_ERR_ARG;
    if ((in_stride & 3) || (out_stride & 3)) return TETRA_ERR_ALIGN;
    if (device_ptrs && (((uintptr_t)in & 3) || ((uintptr_t)out & 3) || ((uintptr_t)biterr & 3))) return TETRA_ERR_ALIGN;
    return TETRA_OK;
}

int tetra_lmac_decode_tch_counted_device(int kind, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                         const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                         uint32_t* d_biterr, void* hip_stream) {
    const int rc = tch_check_args(kind, d_type5, n_blocks, in_stride, d_scramb_init, d_type2, out_stride, d_biterr, true);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const tetra_tch::Kind k = tetra_tch::kind_of(kind);
    const uint32_t* seq = seq_table();
    if (!seq) return TETRA_ERR_NOMEM;
    const int groups = (n_blocks + kLanes - 1) / kLanes;
    const int dec_pairs = k.ng ? (k.type2 + kFlush) / 2 : 0;
    ScratchLease scratch;
    if (dec_pairs)
        if (const int err = scratch.take((size_t)groups * dec_pairs * kLanes * sizeof(uint32_t), nullptr, 0, s)) return err;
    hipLaunchKernelGGL(k_tch_rows, dim3(groups), dim3(kLanes), 0, s, d_type5, n_blocks, in_stride, d_scramb_init, k.ng, k.type2, d_type2, out_stride,
                       scratch.p, dec_pairs, d_n_blocks, d_init_index, seq, g_force_byte_route ? 0 : 1, d_biterr);
    return scratch.launched();
}

int tetra_lmac_decode_tch_batch(int kind, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                uint8_t* type2, int out_stride, uint32_t* biterr, int device) {
    const int rc = tch_check_args(kind, type5, n_blocks, in_stride, scramb_init, type2, out_stride, biterr, false);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_HIP;
    DevMem<uint8_t> d_in, d_out;
    DevMem<uint32_t> d_init, d_biterr;
    const size_t in_bytes = (size_t)n_blocks * in_stride, out_bytes = (size_t)n_blocks * out_stride;
    if (d_in.reserve(in_bytes) != hipSuccess || d_out.reserve(out_bytes) != hipSuccess || d_init.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess ||
        (biterr && d_biterr.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess))
        return TETRA_ERR_NOMEM;
    if (hipMemcpy(d_init, scramb_init, sizeof(uint32_t) * n_blocks, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in, type5, in_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return TETRA_ERR_HIP;
    const int drc = tetra_lmac_decode_tch_counted_device(kind, d_in, n_blocks, nullptr, in_stride, d_init, nullptr, d_out, out_stride,
                                                         biterr ? (uint32_t*)d_biterr : nullptr, nullptr);
    if (drc != TETRA_OK) return drc;
    if (hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    // only the type2 columns: the caller's row padding is left alone
    const int row = tetra_tch::kind_of(kind).type2;
    if (out_stride == row ? hipMemcpy(type2, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess
                          : hipMemcpy2D(type2, out_stride, d_out, out_stride, row, n_blocks, hipMemcpyDeviceToHost) != hipSuccess)
        return TETRA_ERR_HIP;
    if (biterr && hipMemcpy(biterr, d_biterr, sizeof(uint32_t) * n_blocks, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    return TETRA_OK;
}

// ---- include/ext/tetra_tch_soft.h: int8 byte rows -------------------------------------------------------------------------------------
int tetra_lmac_decode_tch_soft_counted_device(int kind, const int8_t* d_soft, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                              const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                              uint32_t* d_biterr, void* hip_stream) {
    if (kind == TETRA_LMAC_T_TCH_7_2) return TETRA_ERR_ARG;                    // not coded: nothing to gain from soft values
    const int rc = tch_check_args(kind, d_soft, n_blocks, in_stride, d_scramb_init, d_type2, out_stride, d_biterr, true);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const tetra_tch::Kind k = tetra_tch::kind_of(kind);
    const uint32_t* seq = seq_table();
    if (!seq) return TETRA_ERR_NOMEM;
    const int groups = (n_blocks + kLanes - 1) / kLanes;
    const int dec_pairs = (k.type2 + kFlush) / 2;
    ScratchLease scratch;
    if (const int err = scratch.take((size_t)groups * dec_pairs * kLanes * sizeof(uint32_t), nullptr, 0, s)) return err;
    hipLaunchKernelGGL(k_tch_rows_soft, dim3(groups), dim3(kLanes), 0, s, d_soft, n_blocks, in_stride, d_scramb_init, k.ng, k.type2, d_type2, out_stride,
                       scratch.p, dec_pairs, d_n_blocks, d_init_index, seq, d_biterr);
    return scratch.launched();
}

int tetra_lmac_decode_tch_soft_batch(int kind, const int8_t* soft5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                     uint8_t* type2, int out_stride, uint32_t* biterr, int device) {
    if (kind == TETRA_LMAC_T_TCH_7_2) return TETRA_ERR_ARG;
    const int rc = tch_check_args(kind, soft5, n_blocks, in_stride, scramb_init, type2, out_stride, biterr, false);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_HIP;
    DevMem<int8_t> d_in;
    DevMem<uint8_t> d_out;
    DevMem<uint32_t> d_init, d_biterr;
    const size_t in_bytes = (size_t)n_blocks * in_stride, out_bytes = (size_t)n_blocks * out_stride;
    if (d_in.reserve(in_bytes) != hipSuccess || d_out.reserve(out_bytes) != hipSuccess || d_init.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess ||
        (biterr && d_biterr.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess))
        return TETRA_ERR_NOMEM;
    if (hipMemcpy(d_init, scramb_init, sizeof(uint32_t) * n_blocks, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_in, soft5, in_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return TETRA_ERR_HIP;
    const int drc = tetra_lmac_decode_tch_soft_counted_device(kind, d_in, n_blocks, nullptr, in_stride, d_init, nullptr, d_out, out_stride,
                                                              biterr ? (uint32_t*)d_biterr : nullptr, nullptr);
    if (drc != TETRA_OK) return drc;
    if (hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    // only the type2 columns: the caller's row padding is left alone
    const int row = tetra_tch::kind_of(kind).type2;
    if (out_stride == row ? hipMemcpy(type2, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess
                          : hipMemcpy2D(type2, out_stride, d_out, out_stride, row, n_blocks, hipMemcpyDeviceToHost) != hipSuccess)
        return TETRA_ERR_HIP;
    if (biterr && hipMemcpy(biterr, d_biterr, sizeof(uint32_t) * n_blocks, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    return TETRA_OK;
}

// ---- include/ext/tetra_tch_nblk.h ------------------------------------------------------------------------------------------------------
// tch_check_args for a coded kind behind the checks of N, the pool and the window table
static int nblk_check_args(int kind, int n, const void* in, int n_rows, int in_stride, const void* init, const void* index, const void* windows,
                           int n_blocks, const void* out, int out_stride, const void* biterr, bool device_ptrs) {
    if (kind != TETRA_LMAC_T_TCH_4_8 && kind != TETRA_LMAC_T_TCH_2_4) return TETRA_ERR_ARG;
    if (!tetra_tch_nblk::valid_n(n) || n_rows < 0) return TETRA_ERR_ARG;
    if (n_blocks > 0 && !windows) return TETRA_ERR_ARG;
    const int rc = tch_check_args(kind, in, n_blocks, in_stride, init, out, out_stride, biterr, device_ptrs);
    if (rc != TETRA_OK) return rc;
    if (device_ptrs && (((uintptr_t)windows & 3) || ((uintptr_t)init & 3) || ((uintptr_t)index & 3))) return TETRA_ERR_ALIGN;
    return TETRA_OK;
}

static int nblk_launch(bool soft, int kind, int n, const void* d_pool, int n_rows, int in_stride, const uint32_t* d_scramb_init,
                       const int32_t* d_init_index, const int32_t* d_windows, int n_blocks, const int32_t* d_n_blocks, uint8_t* d_type2, int out_stride,
                       uint32_t* d_biterr, void* hip_stream) {
    const int rc = nblk_check_args(kind, n, d_pool, n_rows, in_stride, d_scramb_init, d_init_index, d_windows, n_blocks, d_type2, out_stride, d_biterr, true);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const tetra_tch::Kind k = tetra_tch::kind_of(kind);
    const uint32_t* seq = seq_table();
    if (!seq) return TETRA_ERR_NOMEM;
    const int groups = (n_blocks + kLanes - 1) / kLanes;
    const int dec_pairs = (k.type2 + kFlush) / 2;
    ScratchLease scratch;
    if (const int err = scratch.take((size_t)groups * dec_pairs * kLanes * sizeof(uint32_t), nullptr, 0, s)) return err;
    const NblkArgs a{ d_pool, n_rows, in_stride, d_scramb_init, d_init_index, d_windows, n, n_blocks, d_n_blocks, k.ng, k.type2, d_type2, out_stride,
                      scratch.p, dec_pairs, seq, d_biterr };
    if (soft) hipLaunchKernelGGL(k_tch_nblk_soft, dim3(groups), dim3(kLanes), 0, s, a);
    else hipLaunchKernelGGL(k_tch_nblk, dim3(groups), dim3(kLanes), 0, s, a, g_force_byte_route ? 0 : 1);
    return scratch.launched();
}

int tetra_lmac_decode_tch_nblk_device(int kind, int n_interleave, const uint8_t* d_type5, int n_rows, int in_stride,
                                      const uint32_t* d_scramb_init, const int32_t* d_init_index, const int32_t* d_windows, int n_blocks,
                                      const int32_t* d_n_blocks, uint8_t* d_type2, int out_stride, uint32_t* d_biterr, void* hip_stream) {
    return nblk_launch(false, kind, n_interleave, d_type5, n_rows, in_stride, d_scramb_init, d_init_index, d_windows, n_blocks, d_n_blocks, d_type2,
                       out_stride, d_biterr, hip_stream);
}

int tetra_lmac_decode_tch_nblk_soft_device(int kind, int n_interleave, const int8_t* d_soft, int n_rows, int in_stride,
                                           const uint32_t* d_scramb_init, const int32_t* d_init_index, const int32_t* d_windows, int n_blocks,
                                           const int32_t* d_n_blocks, uint8_t* d_type2, int out_stride, uint32_t* d_biterr, void* hip_stream) {
    return nblk_launch(true, kind, n_interleave, d_soft, n_rows, in_stride, d_scramb_init, d_init_index, d_windows, n_blocks, d_n_blocks, d_type2,
                       out_stride, d_biterr, hip_stream);
}

// both host-pointer variants: the pool, its codes and the window table in, the type2 columns and the counts out
static int nblk_batch(bool soft, int kind, int n, const void* pool, int n_rows, int in_stride, const uint32_t* scramb_init, const int32_t* windows,
                      int n_blocks, uint8_t* type2, int out_stride, uint32_t* biterr, int device) {
    const int rc = nblk_check_args(kind, n, pool, n_rows, in_stride, scramb_init, nullptr, windows, n_blocks, type2, out_stride, biterr, false);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_HIP;
    DevMem<uint8_t> d_in, d_out;
    DevMem<uint32_t> d_init, d_biterr;
    DevMem<int32_t> d_win;
    // (an empty pool is allowed: every window is then lost; the device side never reads it)
    const size_t in_bytes = (size_t)(n_rows ? n_rows : 1) * in_stride, out_bytes = (size_t)n_blocks * out_stride;
    const size_t init_bytes = sizeof(uint32_t) * (n_rows ? n_rows : 1), win_bytes = sizeof(int32_t) * (size_t)n_blocks * n;
    if (d_in.reserve(in_bytes) != hipSuccess || d_out.reserve(out_bytes) != hipSuccess || d_init.reserve(init_bytes) != hipSuccess ||
        d_win.reserve(win_bytes) != hipSuccess || (biterr && d_biterr.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess))
        return TETRA_ERR_NOMEM;
    if ((n_rows && (hipMemcpy(d_init, scramb_init, sizeof(uint32_t) * n_rows, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(d_in, pool, (size_t)n_rows * in_stride, hipMemcpyHostToDevice) != hipSuccess)) ||
        hipMemcpy(d_win, windows, win_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return TETRA_ERR_HIP;
    const int drc = nblk_launch(soft, kind, n, d_in, n_rows, in_stride, d_init, nullptr, d_win, n_blocks, nullptr, d_out, out_stride,
                                biterr ? (uint32_t*)d_biterr : nullptr, nullptr);
    if (drc != TETRA_OK) return drc;
    if (hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    // only the type2 columns: the caller's row padding is left alone
    const int row = tetra_tch::kind_of(kind).type2;
    if (out_stride == row ? hipMemcpy(type2, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess
                          : hipMemcpy2D(type2, out_stride, d_out, out_stride, row, n_blocks, hipMemcpyDeviceToHost) != hipSuccess)
        return TETRA_ERR_HIP;
    if (biterr && hipMemcpy(biterr, d_biterr, sizeof(uint32_t) * n_blocks, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    return TETRA_OK;
}

int tetra_lmac_decode_tch_nblk_batch(int kind, int n_interleave, const uint8_t* type5, int n_rows, int in_stride, const uint32_t* scramb_init,
                                     const int32_t* windows, int n_blocks, uint8_t* type2, int out_stride, uint32_t* biterr, int device) {
    return nblk_batch(false, kind, n_interleave, type5, n_rows, in_stride, scramb_init, windows, n_blocks, type2, out_stride, biterr, device);
}

int tetra_lmac_decode_tch_nblk_soft_batch(int kind, int n_interleave, const int8_t* soft5, int n_rows, int in_stride, const uint32_t* scramb_init,
                                          const int32_t* windows, int n_blocks, uint8_t* type2, int out_stride, uint32_t* biterr, int device) {
    return nblk_batch(true, kind, n_interleave, soft5, n_rows, in_stride, scramb_init, windows, n_blocks, type2, out_stride, biterr, device);
}

}  // extern "C"

// Every frame entry point (lmac_impl.hpp): one job table, the kernel the options select, the list launches behind it for the jobs with ranks.
int lmac_impl::decode_frames(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, const FrameOpts& opts, void* hip_stream) {
    const SoftRing* const soft = opts.soft;
    if (soft) {     // a ring of whole aligned words, a power of two in size; the frames' bit numbers and channels
        if (!soft->d_ring || soft->size < 4 || (soft->size & (soft->size - 1)) || ((uintptr_t)soft->d_ring & 3)) return TETRA_ERR_ARG;
        if (src && (!src->d_frame_bitnum || src->frames_per_channel < 1)) return TETRA_ERR_ARG;
    }
    if (!src || !jobs || n_jobs < 0 || n_jobs > TETRA_LMAC_MAX_JOBS) return TETRA_ERR_ARG;
    if (n_jobs == 0) return TETRA_OK;
    if (!src->d_frames || !src->d_frame_type || src->n_frames < 0) return TETRA_ERR_ARG;
    if ((uintptr_t)src->d_frames & 15) return TETRA_ERR_ALIGN;
    JobTable tab = {};
    BiterrTable counts = {};
    int32_t* ranks[TETRA_LMAC_MAX_JOBS] = {};
    bool any_counts = false;
    if (src->n_frames == 0) return TETRA_OK;              // no frames: no row can exist
    tab.src = DevFrames{ src->d_frames, src->d_frame_type, src->d_frame_bitnum, src->d_time_rx, src->d_time, src->frames_per_channel, src->n_frames };
    long long groups_total = 0, scratch_words = 0;
    int n = 0, max_pairs = 0;
    bool any_rm = false;
    DevJob aach[TETRA_LMAC_MAX_JOBS];
    int aach_min_margin[TETRA_LMAC_MAX_JOBS], n_aach = 0;
    // the TCH jobs (tetra_tch.h): a table and a launch of their own behind the others, their scratch behind the others' in the one lease
    JobTable tch = {};
    BiterrTable tch_counts = {};
    long long tch_groups_total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        tetra_lmac_job_t j = jobs[i];
        if (tetra_tch::is_tch(j.type)) {
            // soft-decision TCH is tetra_tch_soft.h's entry point alone; no CRC for a list decoder to aim at (there a job is refused for a
            // rank entry of its own, so that the signalling jobs beside it may be rescued; elsewhere for the array, as ever)
            if (soft ? !opts.soft_tch || (opts.d_rank && opts.d_rank[i]) : opts.d_rank != nullptr) return TETRA_ERR_ARG;
            const tetra_tch::Kind k = tetra_tch::kind_of(j.type);
            if (soft && !k.ng) return TETRA_ERR_ARG;               // TCH/7.2 is not coded: from the packed frames
            uint32_t* const job_counts = opts.d_biterr ? opts.d_biterr[i] : nullptr;
            if (j.max_rows < 0 || (job_counts && !k.ng)) return TETRA_ERR_ARG;
            if ((uintptr_t)job_counts & 3) return TETRA_ERR_ALIGN;
            if (j.max_rows == 0) continue;
            if (!j.d_row_frame || !j.d_type2 || !j.d_crc_ok || !j.d_frame_scramb) return TETRA_ERR_ARG;
            if (j.d_labels && (!src->d_frame_bitnum || !src->d_time_rx || !src->d_time || src->frames_per_channel < 1)) return TETRA_ERR_ARG;
            if (j.out_stride < k.type2) return TETRA_ERR_SIZE;
            if ((j.out_stride & 7) || ((uintptr_t)j.d_type2 & 7)) return TETRA_ERR_ALIGN;
            tch_counts.out[tch.n] = job_counts;
            DevJob& d = tch.job[tch.n++];
            d.row_frame = j.d_row_frame; d.n_rows_dev = j.d_n_rows; d.frame_scramb = j.d_frame_scramb; d.out = j.d_type2; d.crc_ok = j.d_crc_ok;
            d.labels = j.d_labels; d.n_rows = j.max_rows; d.out_stride = j.out_stride; d.layout = kLayoutSchF;
            d.type345 = tetra_tch::kType345; d.type2 = k.type2; d.a = tetra_tch::kInterleaveA;
            d.dec_pairs = k.ng ? (k.type2 + kFlush) / 2 : 0;
            const long long groups = ((long long)j.max_rows + kLanes - 1) / kLanes;
            d.first_group = (int)tch_groups_total;
            d.scratch_base = scratch_words;
            tch_groups_total += groups;
            scratch_words += groups * d.dec_pairs * kLanes;
            if (tch_groups_total > 0x7fffffffLL) return TETRA_ERR_SIZE;
            continue;
        }
        const bool rm = j.type == (TETRA_TPSAP_T_BBK | TETRA_LMAC_JOB_RM3014);       // (the flag on any other type: refused below)
        // the AACH by maximum likelihood on the ring's values (tetra_aach_soft.h): the soft entry point's alone, min_margin in bits 16..25
        const bool ml = j.type >= 0 && (j.type & ~TETRA_LMAC_JOB_AACH_MIN_MARGIN(0x3ff)) == (TETRA_TPSAP_T_BBK | TETRA_LMAC_JOB_RM3014_SOFT);
        const int min_margin = ml ? (j.type >> 16) & 0x3ff : 0;
        if (ml && (!soft || min_margin > TETRA_AACH_SOFT_MAX_MARGIN)) return TETRA_ERR_ARG;
        if (rm || ml) j.type = TETRA_TPSAP_T_BBK;
        if (j.type < 0 || j.type > 5 || j.max_rows < 0) return TETRA_ERR_ARG;
        uint32_t* const job_counts = opts.d_biterr ? opts.d_biterr[i] : nullptr;
        if (job_counts && j.type == TETRA_TPSAP_T_BBK) return TETRA_ERR_ARG;       // the AACH is not convolutionally coded
        if ((uintptr_t)job_counts & 3) return TETRA_ERR_ALIGN;
        int32_t* const job_rank = opts.d_rank ? opts.d_rank[i] : nullptr;
        if (job_rank && j.type == TETRA_TPSAP_T_BBK) return TETRA_ERR_ARG;         // the AACH has no CRC to aim at
        if (const int bad = check_list(job_rank, opts.max_candidates)) return bad;
        if (j.max_rows == 0) continue;
        if (!j.d_row_frame || !j.d_type2 || !j.d_crc_ok) return TETRA_ERR_ARG;
        if (j.type != TETRA_TPSAP_T_SB1 && !j.d_frame_scramb) return TETRA_ERR_ARG;
        if (j.d_labels && (!src->d_frame_bitnum || !src->d_time_rx || !src->d_time || src->frames_per_channel < 1)) return TETRA_ERR_ARG;
        const int layout = layout_for(j.type, j.blk_num, rm);
        if (layout == kLayoutNone) return TETRA_ERR_ARG;       // no burst type carries this (kind, block number)
        const BlkParam& p = blk_param(j.type);
        const bool bbk = layout == kLayoutBbk || layout == kLayoutBbkRm;
        if (soft && bbk && !ml) return TETRA_ERR_ARG;          // the AACH's hard bits are not in the ring: its soft route is the flag above
        any_rm = any_rm || rm;
        if (j.out_stride < (bbk ? 32 : p.type2)) return TETRA_ERR_SIZE;
        if ((j.out_stride & 7) || ((uintptr_t)j.d_type2 & 7)) return TETRA_ERR_ALIGN;
        if (ml) {                                              // a launch of its own behind the decode launch: not in the job table
            DevJob& d = aach[n_aach];
            d = DevJob{};
            d.row_frame = j.d_row_frame; d.n_rows_dev = j.d_n_rows; d.frame_scramb = j.d_frame_scramb; d.out = j.d_type2; d.crc_ok = j.d_crc_ok;
            d.labels = j.d_labels; d.n_rows = j.max_rows; d.out_stride = j.out_stride; d.layout = kLayoutBbk;
            aach_min_margin[n_aach++] = min_margin;
            continue;
        }
        counts.out[n] = job_counts;
        ranks[n] = job_rank;
        any_counts = any_counts || job_counts;
        DevJob& d = tab.job[n++];
        d.row_frame = j.d_row_frame;
        d.n_rows_dev = j.d_n_rows;
        d.frame_scramb = j.type == TETRA_TPSAP_T_SB1 ? nullptr : j.d_frame_scramb;
        d.out = j.d_type2;
        d.crc_ok = j.d_crc_ok;
        d.labels = j.d_labels;
        d.n_rows = j.max_rows;
        d.out_stride = j.out_stride;
        d.layout = layout;
        d.type345 = p.type345; d.type2 = p.type2; d.a = p.a;
        d.dec_pairs = bbk ? 0 : (p.type2 + kFlush) / 2;
        max_pairs = d.dec_pairs > max_pairs ? d.dec_pairs : max_pairs;
        const long long groups = ((long long)j.max_rows + kLanes - 1) / kLanes;
        d.first_group = (int)groups_total;
        d.scratch_base = scratch_words;
        groups_total += groups;
        scratch_words += groups * d.dec_pairs * kLanes;
        if (groups_total > 0x7fffffffLL) return TETRA_ERR_SIZE;
    }
    tab.n = n;
    if (n == 0 && n_aach == 0 && tch.n == 0) return TETRA_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const uint32_t* seq = seq_table();
    if (!seq) return TETRA_ERR_NOMEM;
    // the soft AACH jobs, each a launch of its own (they are queued behind the decode launch: see the end of the function)
    auto launch_aach = [&]() -> int {
        for (int k = 0; k < n_aach; ++k)
            hipLaunchKernelGGL(k_aach_soft_frames, dim3((unsigned)(((long long)aach[k].n_rows + kAachGroupRows - 1) / kAachGroupRows)), dim3(kAachGroupThreads), 0, s,
                               aach[k], tab.src, seq, reinterpret_cast<const uint32_t*>(soft->d_ring), soft->size / 4u, aach_min_margin[k]);
        return n_aach && hipGetLastError() != hipSuccess ? TETRA_ERR_HIP : TETRA_OK;
    };
    if (n == 0 && tch.n == 0) return launch_aach();
    tch.src = tab.src;
    const size_t bytes = (size_t)scratch_words * sizeof(uint32_t);
    ScratchLease scratch;
    if (const int err = scratch_words ? scratch.take(bytes, src->d_workspace, src->workspace_bytes, s) : TETRA_OK) return err;
    // a launch that counts is an instantiation of its own; every other launch is the kernel it was
    const dim3 grid((unsigned)groups_total), block(kLanes);
    if (n == 0) {
        // TCH jobs alone
    } else if (soft) {
        const uint32_t* ring = reinterpret_cast<const uint32_t*>(soft->d_ring);
        if (any_counts) hipLaunchKernelGGL((k_lmac_frames_soft<true, BiterrTable>), grid, block, 0, s, tab, scratch.p, seq, ring, soft->size / 4u, counts);
        else hipLaunchKernelGGL(k_lmac_frames_soft<false>, grid, block, 0, s, tab, scratch.p, seq, ring, soft->size / 4u);
    } else if (any_rm) {
        const uint32_t* rm_tab = rm3014_table();
        if (!rm_tab) { (void)scratch.give_back(); return TETRA_ERR_NOMEM; }
        if (any_counts) hipLaunchKernelGGL((k_lmac_frames<true, true, BiterrTable>), grid, block, 0, s, tab, scratch.p, seq, rm_tab, counts);
        else hipLaunchKernelGGL(k_lmac_frames<true>, grid, block, 0, s, tab, scratch.p, seq, rm_tab);
    } else if (any_counts) {
        hipLaunchKernelGGL((k_lmac_frames<false, true, BiterrTable>), grid, block, 0, s, tab, scratch.p, seq, nullptr, counts);
    } else {
        hipLaunchKernelGGL(k_lmac_frames<false>, dim3((unsigned)groups_total), dim3(kLanes), 0, s, tab, scratch.p, seq, nullptr);
    }
    if (tch.n && soft)
        hipLaunchKernelGGL(k_tch_frames_soft, dim3((unsigned)tch_groups_total), block, 0, s, tch, scratch.p, seq, reinterpret_cast<const uint32_t*>(soft->d_ring),
                           soft->size / 4u, tch_counts);
    else if (tch.n) hipLaunchKernelGGL(k_tch_frames, dim3((unsigned)tch_groups_total), block, 0, s, tch, scratch.p, seq, tch_counts);
    // the jobs with ranks, all in one set of list launches: behind the decode launch, in front of the scratch's hand-back
    RescueTable rt = {};
    for (int k = 0; k < n; ++k) {
        if (!ranks[k]) continue;
        const DevJob& d = tab.job[k];
        RescueJob& a = add_rescue_job(rt, d.n_rows_dev, d.n_rows, d.crc_ok, d.out, d.out_stride, d.labels, counts.out[k], ranks[k], scratch.p + d.scratch_base,
                                      d.dec_pairs, d.type345, d.type2, d.a);
        a.row_frame = d.row_frame; a.frame_scramb = d.frame_scramb; a.layout = d.layout;
    }
    rt.T = opts.max_candidates; rt.src = tab.src; rt.seq_tab = seq;
    if (soft) { rt.ring = reinterpret_cast<const uint32_t*>(soft->d_ring); rt.ring_words = soft->size / 4u; }
    const int list_rc = launch_list(soft ? kFrontSoft : kFrontFrames, rt, s, opts.list_work.d_work, opts.list_work.bytes);
    const int launch_rc = scratch.launched();
    const int aach_rc = launch_aach();
    return list_rc != TETRA_OK ? list_rc : launch_rc != TETRA_OK ? launch_rc : aach_rc;
}

extern "C" {

int tetra_lmac_decode_frames_list_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, int max_candidates,
                                         int32_t* const* d_rank, void* hip_stream) {
    return lmac_impl::decode_frames(src, jobs, n_jobs, lmac_impl::FrameOpts{ nullptr, nullptr, d_rank, max_candidates, {} }, hip_stream);
}

int tetra_lmac_decode_frames_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, void* hip_stream) {
    return lmac_impl::decode_frames(src, jobs, n_jobs, lmac_impl::FrameOpts{}, hip_stream);
}

int tetra_lmac_decode_frames_biterr_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, uint32_t* const* d_biterr,
                                           void* hip_stream) {
    return lmac_impl::decode_frames(src, jobs, n_jobs, lmac_impl::FrameOpts{ nullptr, d_biterr, nullptr, 0, {} }, hip_stream);
}

int tetra_lmac_decode_frames_soft_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, const int8_t* d_ring, uint32_t ring_size,
                                         uint32_t* const* d_biterr, int32_t* const* d_rank, int max_candidates, void* hip_stream) {
    const lmac_impl::SoftRing ring{ d_ring, ring_size };       // (a NULL ring is refused there: never "no ring", the hard route)
    return lmac_impl::decode_frames(src, jobs, n_jobs, lmac_impl::FrameOpts{ &ring, d_biterr, d_rank, max_candidates, {} }, hip_stream);
}

int tetra_lmac_decode_frames_soft_tch_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, const int8_t* d_ring, uint32_t ring_size,
                                             uint32_t* const* d_biterr, int32_t* const* d_rank, int max_candidates, void* hip_stream) {
    const lmac_impl::SoftRing ring{ d_ring, ring_size };
    lmac_impl::FrameOpts opts{ &ring, d_biterr, d_rank, max_candidates, {} };
    opts.soft_tch = true;
    return lmac_impl::decode_frames(src, jobs, n_jobs, opts, hip_stream);
}

size_t tetra_lmac_decode_frames_workspace_bytes(const tetra_lmac_job_t* jobs, int n_jobs) {
    if (!jobs || n_jobs < 0) return 0;
    size_t words = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const tetra_lmac_job_t& j = jobs[i];
        if (tetra_tch::is_tch(j.type) && j.max_rows > 0) {         // tetra_tch.h; TCH/7.2 has no trellis
            const tetra_tch::Kind k = tetra_tch::kind_of(j.type);
            words += (size_t)(((long long)j.max_rows + kLanes - 1) / kLanes) * (k.ng ? (k.type2 + kFlush) / 2 : 0) * kLanes;
            continue;
        }
        if (j.type < 0 || j.type > 5 || j.type == TETRA_TPSAP_T_BBK || j.max_rows <= 0) continue;
        words += (size_t)(((long long)j.max_rows + kLanes - 1) / kLanes) * ((blk_param(j.type).type2 + kFlush) / 2) * kLanes;
    }
    return words * sizeof(uint32_t);
}

int tetra_lmac_rm3014_decode_device(const uint32_t* d_words, int n, uint32_t* d_out_words, uint8_t* d_dist, void* hip_stream) {
    if (n < 0) return TETRA_ERR_ARG;
    if (n == 0) return TETRA_OK;
    if (!d_words || !d_out_words || !d_dist) return TETRA_ERR_ARG;
    if (((uintptr_t)d_words & 3) || ((uintptr_t)d_out_words & 3)) return TETRA_ERR_ALIGN;
    const uint32_t* rm_tab = rm3014_table();
    if (!rm_tab) return TETRA_ERR_NOMEM;
    hipLaunchKernelGGL(k_rm3014, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_words, n, d_out_words, d_dist,
                       rm_tab);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_lmac_rm3014_soft_decode_device(const int8_t* d_soft, int n, int soft_stride, uint32_t* d_out_words, uint8_t* d_dist, uint16_t* d_margin,
                                         void* hip_stream) {
    if (n < 0) return TETRA_ERR_ARG;
    if (n == 0) return TETRA_OK;
    if (!d_soft || soft_stride < 32) return TETRA_ERR_ARG;
    if (((uintptr_t)d_soft & 3) || (soft_stride & 3) || ((uintptr_t)d_out_words & 3) || ((uintptr_t)d_margin & 1)) return TETRA_ERR_ALIGN;
    hipLaunchKernelGGL(k_aach_soft, dim3((unsigned)(((long long)n + kAachGroupRows - 1) / kAachGroupRows)), dim3(kAachGroupThreads), 0,
                       static_cast<hipStream_t>(hip_stream), d_soft, n, soft_stride, d_out_words, d_dist, d_margin);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_lmac_decode_aach_rm3014_device(const uint8_t* d_type5, int n_blocks, int in_stride, const uint32_t* d_scramb_init,
                                         uint8_t* d_type2, int out_stride, int32_t* d_crc_ok, void* hip_stream) {
    const int rc = check_args(TETRA_TPSAP_T_BBK, d_type5, n_blocks, in_stride, d_scramb_init, d_type2, out_stride, d_crc_ok, true);
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    if (out_stride < 32) return TETRA_ERR_ARG;                 // bytes 30 and 31 of a row
    const uint32_t* rm_tab = rm3014_table();
    if (!rm_tab) return TETRA_ERR_NOMEM;
    hipLaunchKernelGGL((k_lmac_bbk<true, const uint32_t*>), dim3((n_blocks + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_type5, n_blocks,
                       in_stride, d_scramb_init, 30, d_type2, out_stride, d_crc_ok, nullptr, nullptr, rm_tab);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_lmac_debug_force_byte_route(int on) {
    const int was = g_force_byte_route ? 1 : 0;
    g_force_byte_route = on != 0;
    return was;
}

// The three tracking entry points: one kernel (k_track), one wavefront per channel.  The slot layout reads its rows as bytes, so it
// takes any stride and row alignment; the compact rows are read as words.
int tetra_lmac_track_scramb_device(const uint8_t* d_sb1_type2, int type2_stride, const int32_t* d_crc_ok, const int32_t* d_valid,
                                   int n_channels, int frames_per_channel, uint32_t* d_chan_scramb, uint32_t* d_row_scramb,
                                   void* hip_stream) {
    if (!d_sb1_type2 || !d_crc_ok || !d_valid || !d_chan_scramb || !d_row_scramb) return TETRA_ERR_ARG;
    if (n_channels < 1 || frames_per_channel < 0 || type2_stride < 60) return TETRA_ERR_ARG;
    if (frames_per_channel == 0) return TETRA_OK;
    hipLaunchKernelGGL((k_track<kRowsSlot, uint32_t>), dim3(n_channels), dim3(kLanes), 0, static_cast<hipStream_t>(hip_stream), d_sb1_type2,
                       type2_stride, d_crc_ok, d_valid, nullptr, nullptr, frames_per_channel, d_chan_scramb, d_row_scramb, nullptr, nullptr,
                       nullptr, nullptr);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_lmac_track_sync_device(const uint8_t* d_sb1_type2, int type2_stride, const int32_t* d_crc_ok, const int32_t* d_valid,
                                 const int32_t* d_n_frames, int n_channels, int frames_per_channel, tetra_lmac_cell_state_t* d_cell,
                                 uint32_t* d_row_scramb, uint32_t* d_row_time_rx, uint32_t* d_row_time, void* hip_stream) {
    if (!d_sb1_type2 || !d_crc_ok || !d_valid || !d_cell || !d_row_scramb) return TETRA_ERR_ARG;
    if (n_channels < 1 || frames_per_channel < 0 || type2_stride < 60) return TETRA_ERR_ARG;
    if (frames_per_channel == 0) return TETRA_OK;
    hipLaunchKernelGGL((k_track<kRowsSlot, tetra_lmac_cell_state_t>), dim3(n_channels), dim3(kLanes), 0, static_cast<hipStream_t>(hip_stream),
                       d_sb1_type2, type2_stride, d_crc_ok, d_valid, d_n_frames, nullptr, frames_per_channel, d_cell, d_row_scramb,
                       d_row_time_rx, d_row_time, nullptr, nullptr);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_lmac_track_sync_lists_device(const uint8_t* d_sb1_type2, int type2_stride, const int32_t* d_crc_ok, const int32_t* d_frame_type,
                                       const int32_t* d_n_frames, const int32_t* d_chan_first_sync, int n_channels, int frames_per_channel,
                                       tetra_lmac_cell_state_t* d_cell, uint32_t* d_row_scramb, uint32_t* d_row_time_rx, uint32_t* d_row_time,
                                       const uint32_t* d_frame_bitnum, tetra_lmac_label_t* d_sb1_labels, void* hip_stream) {
    if (!d_sb1_type2 || !d_crc_ok || !d_frame_type || !d_chan_first_sync || !d_cell || !d_row_scramb) return TETRA_ERR_ARG;
    if (n_channels < 1 || frames_per_channel < 0 || type2_stride < 60 || (d_sb1_labels && !d_frame_bitnum)) return TETRA_ERR_ARG;
    if ((type2_stride & 3) || ((uintptr_t)d_sb1_type2 & 3)) return TETRA_ERR_ALIGN;
    if (frames_per_channel == 0) return TETRA_OK;
    hipLaunchKernelGGL((k_track<kRowsList, tetra_lmac_cell_state_t>), dim3(n_channels), dim3(kLanes), 0, static_cast<hipStream_t>(hip_stream),
                       d_sb1_type2, type2_stride, d_crc_ok, d_frame_type, d_n_frames, d_chan_first_sync, frames_per_channel, d_cell,
                       d_row_scramb, d_row_time_rx, d_row_time, d_frame_bitnum, d_sb1_labels);
    return hipGetLastError() == hipSuccess ? TETRA_OK : TETRA_ERR_HIP;
}

int tetra_lmac_decode_batch(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                            uint8_t* type2, int out_stride, int32_t* crc_ok, int device) {
    return tetra_lmac_decode_batch_biterr(type, type5, n_blocks, in_stride, scramb_init, type2, out_stride, crc_ok, nullptr, device);
}

static int decode_batch(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                        uint8_t* type2, int out_stride, int32_t* crc_ok, uint32_t* biterr, int max_candidates, int32_t* rank, int device);

int tetra_lmac_decode_batch_biterr(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                   uint8_t* type2, int out_stride, int32_t* crc_ok, uint32_t* biterr, int device) {
    return decode_batch(type, type5, n_blocks, in_stride, scramb_init, type2, out_stride, crc_ok, biterr, 0, nullptr, device);
}

int tetra_lmac_decode_batch_list(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                 uint8_t* type2, int out_stride, int32_t* crc_ok, int max_candidates, int32_t* rank, int device) {
    return decode_batch(type, type5, n_blocks, in_stride, scramb_init, type2, out_stride, crc_ok, nullptr, max_candidates, rank, device);
}

static int decode_batch(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                        uint8_t* type2, int out_stride, int32_t* crc_ok, uint32_t* biterr, int max_candidates, int32_t* rank, int device) {
    int rc = check_args(type, type5, n_blocks, in_stride, scramb_init, type2, out_stride, crc_ok, false);
    if (rc == TETRA_OK && (biterr || rank) && type == TETRA_TPSAP_T_BBK) rc = TETRA_ERR_ARG;
    if (rc == TETRA_OK && rank && (max_candidates < 1 || max_candidates > tetra_list::kMaxCandidates)) rc = TETRA_ERR_ARG;
    if (rc != TETRA_OK || n_blocks == 0) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return TETRA_ERR_HIP;
    DevMem<uint8_t> d_in, d_out;
    DevMem<uint32_t> d_init;
    DevMem<int32_t> d_ok;
    DevMem<uint32_t> d_biterr;
    DevMem<int32_t> d_rank;
    if (biterr && d_biterr.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess) return TETRA_ERR_NOMEM;
    if (rank && d_rank.reserve(sizeof(int32_t) * n_blocks) != hipSuccess) return TETRA_ERR_NOMEM;
    const size_t in_bytes = (size_t)n_blocks * in_stride, out_bytes = (size_t)n_blocks * out_stride;
    if (d_in.reserve(in_bytes) != hipSuccess || d_out.reserve(out_bytes) != hipSuccess || d_ok.reserve(sizeof(int32_t) * n_blocks) != hipSuccess)
        return TETRA_ERR_NOMEM;
    if (scramb_init) {
        if (d_init.reserve(sizeof(uint32_t) * n_blocks) != hipSuccess) return TETRA_ERR_NOMEM;
        if (hipMemcpy(d_init, scramb_init, sizeof(uint32_t) * n_blocks, hipMemcpyHostToDevice) != hipSuccess) return TETRA_ERR_HIP;
    }
    if (hipMemcpy(d_in, type5, in_bytes, hipMemcpyHostToDevice) != hipSuccess) return TETRA_ERR_HIP;
    rc = decode_counted(type, d_in, n_blocks, nullptr, in_stride, d_init, nullptr, d_out, out_stride, d_ok, biterr ? (uint32_t*)d_biterr : nullptr,
                        max_candidates, rank ? (int32_t*)d_rank : nullptr, nullptr);
    if (rc != TETRA_OK) return rc;
    if (hipDeviceSynchronize() != hipSuccess) return TETRA_ERR_HIP;
    // only the type2_bits columns: the caller's row padding is left alone
    // (rows without padding: one contiguous copy -- a strided device-to-host copy of many narrow rows crawls)
    const int row = blk_param(type).type2;
    if (out_stride == row ? hipMemcpy(type2, d_out, out_bytes, hipMemcpyDeviceToHost) != hipSuccess
                          : hipMemcpy2D(type2, out_stride, d_out, out_stride, row, n_blocks, hipMemcpyDeviceToHost) != hipSuccess)
        return TETRA_ERR_HIP;
    if (hipMemcpy(crc_ok, d_ok, sizeof(int32_t) * n_blocks, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    if (biterr && hipMemcpy(biterr, d_biterr, sizeof(uint32_t) * n_blocks, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    if (rank && hipMemcpy(rank, d_rank, sizeof(int32_t) * n_blocks, hipMemcpyDeviceToHost) != hipSuccess) return TETRA_ERR_HIP;
    return TETRA_OK;
}

}  // extern "C"

size_t lmac_impl::list_work_bytes(const tetra_lmac_job_t* jobs, int n_jobs) {
    long long tiles = 0, rows = 0;
    for (int i = 0; i < n_jobs; ++i) {
        if (jobs[i].max_rows <= 0 || (jobs[i].type & 0xff) == TETRA_TPSAP_T_BBK) continue;
        tiles += (jobs[i].max_rows + kListTile - 1) / kListTile;
        rows += jobs[i].max_rows;
    }
    return sizeof(int) * list_words(tiles, rows);
}
