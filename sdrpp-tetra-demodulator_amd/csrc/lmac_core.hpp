// lmac_core.hpp -- lane-level code of the batched lower-MAC channel decoder (include/tetra_lmac.h).
//
// One lane decodes one block.  The same source is compiled twice: by hipcc into the gfx950 kernels (tetra_lmac.hip, the
// accessors hit LDS and global memory) and by g++ (-DTETRA_HOST_EMUL) into tests/emul, where it is checked against the
// reference-built primitives without a GPU.  Everything is integer work, so "same source" means "same results".  What the
// kernels share with the emulation: the block table and layout map (blk_param, layout_for), the cooperative front end of byte
// rows (needs_byte_route, pack_units, staged_row) and its byte route (descramble_chunk), the scrambling sequence (lane_sequence,
// descramble_words), the blocks cut from packed frames (frame_block, bbk_bits), the block front ends composed of those, one per source
// (frame_lookup, load_frame, frame_hard_block, byte_row_block; soft_core.hpp's soft_block), forward recursion + traceback + CRC
// (decode_hard; soft_core.hpp's decode_soft ends in the same traceback), the channel bit-error count of a decoded block
// (reencode_errors, opt-in: include/ext/tetra_biterr.h) and the write-back of both row widths (write_rows).
//
// Restated from the reference (src/decoder/src/lower_mac/), not copied:
//   * scrambler        tetra_scramb.c:34-51 (Fibonacci LFSR, taps 32 26 23 22 16 12 11 10 8 7 5 4 2 1, shifts right, new
//                      bit enters at bit 31) -- here the tap XOR is one AND + parity;
//   * soft mapping     viterbi.c:12-23 (0 -> +127, 0xff -> 0, else -> -127) -- here in units of 127 as a 2-bit signed class;
//   * deinterleaver    tetra_interleave.c:36-39, :51-59: type3[i-1] = type4[(a*i) % K], i = 1..K -- here a running index;
//   * depuncturer      tetra_conv_enc.c:229-251 with punct_2_3 (:131-137, P = {0,1,2,5}, t = 3, period 8): type-3 bit j lands
//                      on mother-code bit 8*((j-1)/3) + P[1 + (j-1)%3] - 1, i.e. bits 0,1 (g1,g2) of every even trellis
//                      step and bit 0 (g1) of every odd one; all others are erasures (metric contribution 0);
//   * decoder          osmo_conv.c: K = 5, N = 4, 16 states, reg bit 3 = newest input bit (:370-392); predecessors of
//                      states i and i+8 are 2i and 2i+1 (:63-95); branch metric m_i = sum_q soft[q] * (1 - 2*g_q) for the
//                      transition 2i --0--> i (:121-133), the other three transitions of the butterfly are -m, -m, +m
//                      because every generator has the D^0 and D^4 terms; ties pick the even predecessor; path metric
//                      of state 0 starts 127*4*5 ahead (:528); CONV_TERM_FLUSH runs K-1 = 4 extra steps (:678-679)
//                      on zero soft bits (viterbi.c:8) and tracebacks from state 0 (:567-612).
//     The reference keeps int16 path metrics and subtracts the minimum every 59 steps (:137-153, :642); with the
//     rate-2/3 depunctured input at most two soft values per step are non-zero, so its sums stay far inside int16 and
//     renormalisation never changes a comparison.  Here the metrics are kept in units of 127 (all soft values are
//     0 or +-127), two per register in packed int16 lanes, without renormalisation: same decisions.
//   * generators       EN 300 392-2 8.2.3.1.1 (tetra_conv_enc.c:45-60 conv_enc_in_bit): g1 = 1+D+D^4, g2 = 1+D^2+D^3+D^4,
//                      g3 = 1+D+D^2+D^4, g4 = 1+D+D^3+D^4.  With i = (d0 d1 d2) the three newer delay bits of the even
//                      predecessor and input 0: g1 = d0, g2 = d1^d2 (g3, g4 only ever meet erasures here).
//   * CRC              crc_simple.c:59-77, :103-106: CRC16-CCITT (0x1021) over the bits, start 0xffff, good = 0x1d0f.
// The SB1 tracker's scalar pieces (SYNC-PDU fields, scrambling code, TDMA clock) are at the end.
#pragma once

#include <stdint.h>

#include "demux_core.hpp"

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define LM_FN __device__ __forceinline__
#else
#define LM_FN static inline
#endif
// (member functions of the defaulted hooks below)
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define LM_MEM __device__ __forceinline__
#else
#define LM_MEM inline
#endif

namespace tetra_lmac {

// bit (32 - y) for every tap y of the reference's ST(x, y) = x >> (32 - y)
constexpr uint32_t tap_bit(int y) { return 1u << (32 - y); }
constexpr uint32_t kScrambTaps = tap_bit(32) | tap_bit(26) | tap_bit(23) | tap_bit(22) | tap_bit(16) | tap_bit(12) | tap_bit(11) |
                                 tap_bit(10) | tap_bit(8) | tap_bit(7) | tap_bit(5) | tap_bit(4) | tap_bit(2) | tap_bit(1);
constexpr uint32_t kScrambInitSb1 = 3;   // SCRAMB_INIT, tetra_scramb.h:14
constexpr uint32_t kCrcOk = 0x1d0f;      // TETRA_CRC_OK, tetra_common.h:330
constexpr int kFlush = 4;                // K - 1
constexpr int kMaxType345 = 432;
constexpr int kMaxType2 = 288;

// tetra_blk_param[], tetra_lower_mac.c:58-105 (values of EN 300 392-2 table 8.x / 8.2.4.1), by TETRA_TPSAP_T_*
struct BlkParam { int type345, type2, type1, a, crc; };
constexpr BlkParam kBlkParam[6] = {
    { 120, 80, 60, 11, 1 },     // SB1
    { 216, 144, 124, 101, 1 },  // SB2
    { 216, 144, 124, 101, 1 },  // NDB
    { 30, 30, 14, 0, 0 },       // BBK
    { 168, 112, 92, 13, 1 },    // SCH/HU
    { 432, 288, 268, 103, 1 },  // SCH/F
};
constexpr const BlkParam& blk_param(int type) { return kBlkParam[type]; }

LM_FN uint32_t lfsr_next(uint32_t& lfsr) {
    const uint32_t bit = (uint32_t)__builtin_popcount(lfsr & kScrambTaps) & 1u;
    lfsr = (lfsr >> 1) | (bit << 31);
    return bit;
}

// bit-field extracts (one instruction each on the device)
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
LM_FN uint32_t bfe_u(uint32_t x, uint32_t off, uint32_t width) { return __builtin_amdgcn_ubfe(x, off, width); }
LM_FN uint32_t bfe_mask(uint32_t x, uint32_t off) { return (uint32_t)__builtin_amdgcn_sbfe((int)x, off, 1u); }     // bit (off & 31) -> 0 / 0xffffffff
#else
LM_FN uint32_t bfe_u(uint32_t x, uint32_t off, uint32_t width) { return (x >> off) & ((1u << width) - 1u); }
LM_FN uint32_t bfe_mask(uint32_t x, uint32_t off) { return 0u - ((x >> (off & 31u)) & 1u); }
#endif

// 2-bit signed class of a descrambled byte: +1 (strong 0), 0 (erasure), -1 = 0b11 (strong 1)
LM_FN uint32_t soft_class(uint32_t v) { return v == 0u ? 1u : (v == 0xffu ? 0u : 3u); }

// Descrambles up to 64 bits of one row (a staging chunk) and packs the soft classes 16 per word.  `remaining` = type-5
// bits left in the row from the start of this chunk (a multiple of 4 for every coded block kind); ld4(d) returns bytes
// 4d..4d+3 of the chunk (little endian); st(w, word) receives chunk word w = classes of chunk bits 16w..16w+15 (2 bits
// each, bit 16w+u at bits 2u..2u+1).  Returns the LFSR state for the next chunk.
template <class Ld4, class St>
LM_FN uint32_t descramble_chunk(int remaining, uint32_t lfsr, Ld4 ld4, St st) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (16 * w < remaining) {
            uint32_t word = 0;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const bool live = (16 * w + 4 * d) < remaining;
                const uint32_t four = live ? ld4(4 * w + d) : 0u;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t bit = lfsr_next(lfsr);
                    const uint32_t v = ((four >> (8 * b)) & 0xffu) ^ bit;
                    const uint32_t c = live ? soft_class(v) : 0u;
                    word |= c << (2 * (4 * d + b));
                }
            }
            st(w, word);
        }
    }
    return lfsr;
}

// ---- clean rows (every byte 0 or 1: what this library's own demultiplexer writes), round 6 -----------------------------------
// The byte-serial route above costs ~12 vector instructions per type-5 bit (an LFSR step + a three-way classification per byte)
// and is what ANY input needs.  A row of plain bits stays bits: pack the bytes 32 to a word, XOR whole words of the scrambling
// sequence, and let the forward recursion pick its three bits per step pair straight from those words (no classes, no erasures).
// The sequence of a 32-bit code is linear in the code (the LFSR has no constant term), so it is the XOR of four table rows indexed
// by the code's bytes: seq_tab[t][byte][w] = word w of the sequence the code (byte << 8 t) generates (kSeqWords words = 448 bits,
// padded to kSeqStride); the host fills the table once per device with scramb_sequence_table below.
// Bit order: type-5 bit i sits at bit 31 - (i & 31) of word i >> 5 -- the order of the burst synchroniser's packed frames, so that
// a block cut out of a packed frame (decode straight from frames) needs no reversal.
constexpr int kSeqWords = (kMaxType345 + 31) / 32;      // 14
constexpr int kSeqStride = 16;
inline void scramb_sequence_words(uint32_t code, uint32_t* words) {
    uint32_t lfsr = code;
    for (int w = 0; w < kSeqWords; ++w) {
        uint32_t v = 0;
        for (int b = 0; b < 32; ++b) {
            const uint32_t bit = (uint32_t)__builtin_popcount(lfsr & kScrambTaps) & 1u;
            lfsr = (lfsr >> 1) | (bit << 31);
            v |= bit << (31 - b);
        }
        words[w] = v;
    }
}
inline void scramb_sequence_table(uint32_t* tab) {       // [4][256][kSeqStride]
    for (int t = 0; t < 4; ++t)
        for (int b = 0; b < 256; ++b) {
            uint32_t* row = tab + ((size_t)t * 256 + b) * kSeqStride;
            scramb_sequence_words((uint32_t)b << (8 * t), row);
            for (int w = kSeqWords; w < kSeqStride; ++w) row[w] = 0;
        }
}
// four bytes 0 / 1 -> a nibble, byte 0 (the first bit) at bit 3
LM_FN uint32_t pack4(uint32_t v) { return (v * 0x08040201u) >> 24; }

struct U2 { uint32_t x, y; };
struct U4 { uint32_t x, y, z, w; };
constexpr int kLanes = 64;                 // a workgroup is one wavefront, a block per lane
constexpr int kChunkDwords = 16;           // 64 type-5 bits per row per staging chunk
constexpr int kStageWords = kChunkDwords + 1;      // a staged row; odd: conflict-free column reads
constexpr int kClsWords = (kMaxType345 + 15) / 16;     // 27: a block as soft classes, 16 per word (descramble_chunk)

// q = i / units by a multiply and a shift, for the flattened (row, unit) index spaces of the front end and the write-back.  Exact for
// every units <= 64 and i < 64 * units (tests/test_lmac.py checks that whole domain against the division).
LM_FN uint32_t unit_inverse(int units) { return ((1u << 20) + (uint32_t)units - 1u) / (uint32_t)units; }
LM_FN int unit_row(int i, uint32_t inv) { return (int)(((uint32_t)i * inv) >> 20); }
// rows that 8-byte accesses can address
LM_FN bool rows_wide(const void* p, int stride) { return !(stride & 7) && !((uintptr_t)p & 7); }
// The packed front end is not for this launch: no sequence table (the byte route forced), rows that are not 8-byte aligned, or rows that
// do not fit the unit -> row map (64 units).
LM_FN bool needs_byte_route(const void* seq_tab, const void* p, int stride) { return seq_tab == nullptr || (stride & 7) || ((uintptr_t)p & 7) || stride > 512; }

// The cooperative front end, the lane's share.  The workgroup's rows_here rows are one contiguous run of rows_here * in_stride bytes:
// it is read ONCE, 8 bytes per lane and 512 contiguous bytes per load instruction (ld8(u) = bytes 8u .. 8u+7 of the run); each unit's
// 8 bytes become 8 bits, dropped as one byte into the row's packed words (st(at, byte): byte `at` of the staged words
// [kLanes][kStageWords]).  Returns non-zero if any byte the lane met is not 0 / 1: then the whole workgroup has to take the byte route.
template <class Ld8, class St>
LM_FN uint32_t pack_units(int lane, int rows_here, int in_stride, int type345, Ld8 ld8, St st) {
    const int units_per_row = in_stride >> 3, total_units = rows_here * units_per_row;
    const uint32_t inv = unit_inverse(units_per_row);
    uint32_t dirty = 0;
    for (int u = lane; u < total_units; u += kLanes) {
        const int r = unit_row(u, inv), j = u - r * units_per_row;      // row, byte of its packed bits
        if (8 * j < type345) {
            const U2 d = ld8(u);
            dirty |= (d.x | d.y) & 0xfefefefeu;
            // type-5 bits 8j .. 8j+7, first bit most significant; byte j of the row's bit string sits in word j / 4 at bits 31 - 8 (j % 4) ..
            st((size_t)r * (4 * kStageWords) + (j & ~3) + (3 - (j & 3)), (uint8_t)((pack4(d.x) << 4) | pack4(d.y)));
        }
    }
    return dirty;
}
// ... then every lane picks up its own row: ld(w) = staged word w of the lane's row (bytes behind the row's last bit were never written)
template <class Ld>
LM_FN void staged_row(int type345, Ld ld, uint32_t xb[kSeqWords]) {
#pragma unroll
    for (int w = 0; w < kSeqWords; ++w) xb[w] = 32 * w < type345 ? ld(w) : 0u;
    if (type345 & 31) xb[type345 >> 5] &= ~(0xffffffffu >> (type345 & 31));
}
// The lane's scrambling sequence: the four table rows the code's bytes select, XORed.  rows(t, byte)[g] = words 4g .. 4g+3 of
// seq_tab[t][byte] as .x .y .z .w (one 16-byte load on the device); st(w, word) receives every word of the groups the block reaches,
// a group that no bit of it reaches is not loaded.
template <class Rows, class St>
LM_FN void lane_sequence(int type345, uint32_t code, Rows rows, St st) {
    const auto r0 = rows(0, code & 0xffu), r1 = rows(1, (code >> 8) & 0xffu), r2 = rows(2, (code >> 16) & 0xffu), r3 = rows(3, code >> 24);
#pragma unroll
    for (int g = 0; g < (kSeqWords + 3) / 4; ++g) {
        if (128 * g < type345) {
            const auto s0 = r0[g], s1 = r1[g], s2 = r2[g], s3 = r3[g];
            const uint32_t w[4] = { s0.x ^ s1.x ^ s2.x ^ s3.x, s0.y ^ s1.y ^ s2.y ^ s3.y, s0.z ^ s1.z ^ s2.z ^ s3.z, s0.w ^ s1.w ^ s2.w ^ s3.w };
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < kSeqWords) st(4 * g + k, w[k]);
        }
    }
}
// the packed rows' descrambling: st(w, word) = type-4 bits 32w .. 32w+31, for the words the block reaches
template <class Rows, class St>
LM_FN void descramble_words(int type345, uint32_t code, const uint32_t xb[kSeqWords], Rows rows, St st) {
    lane_sequence(type345, code, rows, [&](int w, uint32_t word) { if (32 * w < type345) st(w, xb[w] ^ word); });
}

// ---- blocks straight from the burst synchroniser's packed frames (16 words, first bit most significant) ---------------------------
constexpr int kFrameWords = 16;
// 32 bits of a frame from burst bit s on; bits past the 512th read as zero.  (s is a constant wherever this is called: the block
// kind of a job selects one of a handful of literal layouts, and the loops around it are unrolled.)
LM_FN uint32_t frame_window(const uint32_t fw[kFrameWords], int s) {
    const int w = s >> 5, sh = s & 31;
    const uint32_t hi = w < kFrameWords ? fw[w] : 0u, lo = w + 1 < kFrameWords ? fw[w + 1] : 0u;
    return sh ? (hi << sh) | (lo >> (32 - sh)) : hi;
}
// the type-5 bits of a block = burst bits [off0, off0 + len0) then [off1, off1 + len1) (tetra_burst.c:343-393), as packed words
// (bit i at bit 31 - (i & 31) of word i >> 5), zero behind the block
LM_FN void extract_block(const uint32_t fw[kFrameWords], int off0, int len0, int off1, int len1, uint32_t xb[kSeqWords]) {
    const int total = len0 + len1;
#pragma unroll
    for (int v = 0; v < kSeqWords; ++v) {
        const int start = 32 * v;
        uint32_t x = 0;
        if (start < total) {
            if (start + 32 <= len0) x = frame_window(fw, off0 + start);
            else if (start >= len0) x = frame_window(fw, off1 + start - len0);
            else x = (frame_window(fw, off0 + start) & ~(0xffffffffu >> (len0 - start))) | (frame_window(fw, off1) >> (len0 - start));
            if (total - start < 32) x &= ~(0xffffffffu >> (total - start));
        }
        xb[v] = x;
    }
}

// where a kind's bits sit in its burst (demux_core::pieces_for), as literal layouts so that every shift is a constant
enum { kLayoutSb1 = 0, kLayoutSb2, kLayoutNdb1, kLayoutNdb2, kLayoutSchF, kLayoutBbk, kLayoutNone,
       kLayoutBbkRm };      // the AACH decoded with its Reed-Muller code (only the kernel's RM instantiation meets it)
// the layout of block blk_num of a kind in the downlink burst that carries it; kLayoutNone: no burst carries this (kind, block number)
// (SCH/HU is an uplink block)
constexpr int layout_for(int tpsap, int blk_num, bool rm) {
    switch (tpsap) {
        case TETRA_TPSAP_T_SB1: return blk_num == 1 ? kLayoutSb1 : kLayoutNone;
        case TETRA_TPSAP_T_SB2: return blk_num == 2 ? kLayoutSb2 : kLayoutNone;
        case TETRA_TPSAP_T_NDB: return blk_num == 1 ? kLayoutNdb1 : blk_num == 2 ? kLayoutNdb2 : kLayoutNone;
        case TETRA_TPSAP_T_BBK: return rm ? kLayoutBbkRm : kLayoutBbk;
        case TETRA_TPSAP_T_SCH_F: return kLayoutSchF;
        default: return kLayoutNone;
    }
}
template <int TRAIN, int TPSAP, int BLK>
LM_FN void cut(const uint32_t fw[kFrameWords], int frame_type, uint32_t xb[kSeqWords]) {
    const demux_core::Pieces p = demux_core::pieces_for(TRAIN, TPSAP, BLK);
    extract_block(fw, p.off0, p.len0, p.off1, p.len1, xb);
    if (frame_type != TRAIN) {          // a listed frame of another burst type: the demultiplexer's all-zero row
#pragma unroll
        for (int v = 0; v < kSeqWords; ++v) xb[v] = 0;
    }
}
LM_FN void frame_block(int layout, const uint32_t fw[kFrameWords], int frame_type, uint32_t xb[kSeqWords]) {
    switch (layout) {
        case kLayoutSb1: cut<TETRA_TRAIN_SYNC, TETRA_TPSAP_T_SB1, 1>(fw, frame_type, xb); break;
        case kLayoutSb2: cut<TETRA_TRAIN_SYNC, TETRA_TPSAP_T_SB2, 2>(fw, frame_type, xb); break;
        case kLayoutNdb1: cut<TETRA_TRAIN_NORM_2, TETRA_TPSAP_T_NDB, 1>(fw, frame_type, xb); break;
        case kLayoutNdb2: cut<TETRA_TRAIN_NORM_2, TETRA_TPSAP_T_NDB, 2>(fw, frame_type, xb); break;
        case kLayoutSchF: cut<TETRA_TRAIN_NORM_1, TETRA_TPSAP_T_SCH_F, 0>(fw, frame_type, xb); break;
        default:
#pragma unroll
            for (int v = 0; v < kSeqWords; ++v) xb[v] = 0;
    }
}
// the 30 AACH bits of a frame (SYNC: one piece, NORM_1 / NORM_2: two), first bit most significant; 0 for any other frame type
LM_FN uint32_t bbk_bits(const uint32_t fw[kFrameWords], int frame_type) {
    uint32_t xs[kSeqWords], xn[kSeqWords];
    const demux_core::Pieces ps = demux_core::pieces_for(TETRA_TRAIN_SYNC, TETRA_TPSAP_T_BBK, 0);
    const demux_core::Pieces pn = demux_core::pieces_for(TETRA_TRAIN_NORM_1, TETRA_TPSAP_T_BBK, 0);
    extract_block(fw, ps.off0, ps.len0, ps.off1, ps.len1, xs);
    extract_block(fw, pn.off0, pn.len0, pn.off1, pn.len1, xn);
    return frame_type == TETRA_TRAIN_SYNC ? xs[0] : ((frame_type == TETRA_TRAIN_NORM_1 || frame_type == TETRA_TRAIN_NORM_2) ? xn[0] : 0u);
}
LM_FN uint32_t rev32(uint32_t x) {
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
    return __builtin_bitreverse32(x);
#else
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
    return r;
#endif
}
LM_FN uint32_t spread4(uint32_t nib);
// bits 4k..4k+3 of a first-bit-most-significant word as four bytes, first bit in the low byte
LM_FN uint32_t bbk_bytes(uint32_t y, int k) { return spread4(rev32(y << (4 * k)) & 0xfu); }

// ---- block front ends: how a lane turns its source into the descrambled type-4 block, one function per source ------------------------
// Every decode kernel, the rescue behind it (which has to stage a block exactly as its decode launch did: tetra_list.h) and the host
// emulation call these; none of them composes the steps above itself.  (The soft source is soft_core.hpp's soft_block; k_lmac_decode's
// cooperative route stages its chunks through LDS between barriers and keeps its own loop around descramble_chunk.)
// A listed row's frame and scrambling code: a list entry outside [0, n_frames) -- a caller's slip -- reads the nearest frame instead of
// memory that is not there; frame_scramb NULL: SB1's fixed code.
struct FrameRef { int f; uint32_t code; };
LM_FN FrameRef frame_lookup(int listed, int n_frames, const uint32_t* frame_scramb) {
    const int lo = listed > 0 ? listed : 0, f = lo < n_frames - 1 ? lo : n_frames - 1;
    return FrameRef{ f, frame_scramb ? frame_scramb[f] : kScrambInitSb1 };
}
// the lane's packed frame: ld16(g) = words 4g .. 4g+3 of the frame as .x .y .z .w (one 16-byte load on the device)
template <class Ld16>
LM_FN void load_frame(Ld16 ld16, uint32_t fw[kFrameWords]) {
#pragma unroll
    for (int g = 0; g < kFrameWords / 4; ++g) {
        const auto v = ld16(g);
        fw[4 * g] = v.x; fw[4 * g + 1] = v.y; fw[4 * g + 2] = v.z; fw[4 * g + 3] = v.w;
    }
}
// Hard block from a packed frame: the layout's bit ranges, descrambled; st(w, word) as descramble_words'.  J: the job, anything with
// .layout and .type345 (an entry of a kernel's job table, or a BlockKind); frame_type(): the frame's burst type.  A pointer and an
// accessor so that each of these loads happens where its value is used: a reference parameter tells the compiler that the whole job
// can be read at once, it then hoists and merges the job's loads, and every frame kernel's schedule changes.
struct BlockKind { int layout, type345; };
template <class Job, class FrameType, class Rows, class St>
LM_FN void frame_hard_block(const Job* J, uint32_t code, const uint32_t fw[kFrameWords], FrameType frame_type, Rows rows, St st) {
    uint32_t xb[kSeqWords];
    frame_block(J->layout, fw, frame_type(), xb);
    descramble_words(J->type345, code, xb, rows, st);
}
// byte row read by its own lane, any byte values: ld4(d) = bytes 4d .. 4d+3 of the row; st(w, word) = soft classes of bits 16w .. 16w+15
template <class Job, class Ld4, class St>
LM_FN void byte_row_block(const Job* J, uint32_t code, Ld4 ld4, St st) {
    uint32_t lfsr = code;
    for (int c0 = 0; c0 < J->type345 >> 2; c0 += kChunkDwords)      // the cooperative route's 64-bit staging chunks
        lfsr = descramble_chunk(J->type345 - 4 * c0, lfsr, [&](int d) { return ld4(c0 + d); }, [&](int w, uint32_t word) { st(c0 / 4 + w, word); });
}

// ---- packed 16-bit lanes: two path metrics per 32-bit register (v_pk_add_i16 / v_pk_sub_i16 / v_pk_max_i16) --------
// In units of 127 a path metric never leaves [-2*292, 20 + 2*292], so int16 needs no renormalisation at all.
// pk_lo2 / pk_hi2 / pk_swap feed a packed operation and cost nothing on the device: the compiler folds them into the operation's
// op_sel / op_sel_hi operand modifiers.
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
typedef short Pk __attribute__((ext_vector_type(2)));
LM_FN Pk pk_make(int lo, int hi) { Pk r; r.x = (short)lo; r.y = (short)hi; return r; }
LM_FN Pk pk_add(Pk a, Pk b) { return a + b; }
LM_FN Pk pk_sub(Pk a, Pk b) { return a - b; }
LM_FN Pk pk_max(Pk a, Pk b) { return __builtin_elementwise_max(a, b); }
LM_FN Pk pk_lo2(Pk x) { return __builtin_shufflevector(x, x, 0, 0); }
LM_FN Pk pk_hi2(Pk x) { return __builtin_shufflevector(x, x, 1, 1); }
LM_FN Pk pk_swap(Pk x) { return __builtin_shufflevector(x, x, 1, 0); }
LM_FN uint32_t pk_bits(Pk a) { return __builtin_bit_cast(uint32_t, a); }
LM_FN Pk pk_from_bits(uint32_t v) { return __builtin_bit_cast(Pk, v); }
// v_perm_b32: byte k of the result = byte sel[k] of the eight bytes { hi (7..4), lo (3..0) }
LM_FN uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
// bits of a where keep is set, bits of b elsewhere -- as v_bitop3_b32 (truth table 0xe4), which issues at twice the rate of the
// v_bfi_b32 the compiler picks for the same expression (profiles/r06/r06_o_int_rate.jsonl)
LM_FN uint32_t select_bits(uint32_t a, uint32_t b, uint32_t keep) { return __builtin_amdgcn_bitop3_b32(a, b, keep, 0xe4); }
#else
struct Pk { int16_t x, y; };
LM_FN Pk pk_make(int lo, int hi) { return Pk{ (int16_t)lo, (int16_t)hi }; }
LM_FN Pk pk_add(Pk a, Pk b) { return Pk{ (int16_t)(a.x + b.x), (int16_t)(a.y + b.y) }; }
LM_FN Pk pk_sub(Pk a, Pk b) { return Pk{ (int16_t)(a.x - b.x), (int16_t)(a.y - b.y) }; }
LM_FN Pk pk_max(Pk a, Pk b) { return Pk{ a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y }; }
LM_FN Pk pk_lo2(Pk x) { return Pk{ x.x, x.x }; }
LM_FN Pk pk_hi2(Pk x) { return Pk{ x.y, x.y }; }
LM_FN Pk pk_swap(Pk x) { return Pk{ x.y, x.x }; }
LM_FN uint32_t pk_bits(Pk a) { return (uint32_t)(uint16_t)a.x | ((uint32_t)(uint16_t)a.y << 16); }
LM_FN Pk pk_from_bits(uint32_t v) { return Pk{ (int16_t)(v & 0xffffu), (int16_t)(v >> 16) }; }
LM_FN uint32_t select_bits(uint32_t a, uint32_t b, uint32_t keep) { return (a & keep) | (b & ~keep); }
LM_FN uint32_t perm_b32(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint64_t all = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) r |= (uint32_t)((all >> (8 * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
    return r;
}
#endif

// Path metrics of the 16 states: R[i] = (S[i], S[i + 8]).  Butterfly i has predecessors 2i (even) and 2i + 1 (odd) and produces
// states i and i + 8 -- exactly one register -- from one half each of R[2i & 7] and R[(2i + 1) & 7]: with the halves broadcast by
// operand modifiers a step is 8 x (add, subtract, maximum, difference) and not one move (round 6; until then (S[4k], S[4k+2]) /
// (S[4k+1], S[4k+3]) pairs and eight permutes per step to re-pair the results).
struct PathMetrics { Pk R[8]; };

// One add-compare-select step.  Mm[i] = (m_i, -m_i), m_i = branch metric of the transition 2i --0--> i (the other three transitions
// of the butterfly are -m, -m, +m).  D[i] = (difference into state i, into state i + 8): negative <=> the odd predecessor is
// strictly better (ties keep the even one).
LM_FN void acs_step(PathMetrics& pm, const Pk Mm[8], Pk D[8]) {
    Pk N[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const Pk a = pm.R[(2 * i) & 7], b = pm.R[(2 * i + 1) & 7];
        const Pk e = pk_add(i < 4 ? pk_lo2(a) : pk_hi2(a), Mm[i]);      // S[2i] + m, S[2i] - m
        const Pk o = pk_sub(i < 4 ? pk_lo2(b) : pk_hi2(b), Mm[i]);      // S[2i+1] - m, S[2i+1] + m
        N[i] = pk_max(e, o);
        D[i] = pk_sub(e, o);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) pm.R[i] = N[i];
}

// The 2 x 16 decisions of a step pair as one word: state s of the even step at bit 2 (15 - s) + 1, of the odd step at bit
// 2 (15 - s); 1 = the state took its odd predecessor.  A permute gathers the four sign bytes of D[k] and D[k + 4] (states k, k + 4,
// k + 8, k + 12 -> bytes 3, 2, 1, 0); the eight gathered words are then merged from bit 7 of every byte downwards, a shift and a
// bit-field insert each: 22 instructions per step pair (until round 6 a shift and a masked OR per difference register: 38).
LM_FN uint32_t decision_word(const Pk De[8], const Pk Do[8]) {
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t pe = perm_b32(pk_bits(De[k]), pk_bits(De[k + 4]), 0x05010703u);
        const uint32_t po = perm_b32(pk_bits(Do[k]), pk_bits(Do[k + 4]), 0x05010703u);
        const uint32_t keep_e = 0x01010101u * (0xffu & ~(0xffu >> (2 * k))), keep_o = 0x01010101u * (0xffu & ~(0xffu >> (2 * k + 1)));
        w = select_bits(w, pe >> (2 * k), keep_e);          // bits 7 - 2k and below of every byte from pe (below: overwritten next)
        w = select_bits(w, po >> (2 * k + 1), keep_o);
    }
    return w;
}

// Branch metrics of a step pair: P = (p, -p), Q = (q, -q) for the even step (g1 -> sa, g2 -> sb; butterfly i = (d0 d1 d2):
// sign(g1) = d0, sign(g2) = d1 ^ d2, so with p = sa + sb, q = sa - sb the metrics are m_0..7 = p, q, q, p, -q, -p, -p, -q),
// C = (sc, -sc) for the odd step (g1 -> sc only: m_0..3 = sc, m_4..7 = -sc).
struct Bm { Pk P, Q, C; };
LM_FN Bm bm_from_classes(int sa, int sb, int sc) {
    return Bm{ pk_make(sa + sb, -(sa + sb)), pk_make(sa - sb, sb - sa), pk_make(sc, -sc) };
}
// the same from three plain bits given as masks (0 -> class +1, all ones -> class -1): five + two instructions
LM_FN Bm bm_from_masks(uint32_t ma, uint32_t mb, uint32_t mc) {
    const uint32_t k = 0xfffe0002u;                                     // (2, -2)
    const Pk A = pk_from_bits(ma & k), B = pk_from_bits(mb & k);
    return Bm{ pk_sub(pk_sub(pk_from_bits(k), A), B), pk_sub(B, A), pk_from_bits(0xffff0001u ^ (mc & 0xfffefffeu)) };
}

// the interleaver's running index (a * i) % K, i = 1, 2, ...: returns the current position and advances (a < K for every kind)
LM_FN int interleave_next(int& pos, int a, int K) {
    const int p = pos;
    pos += a;
    pos = pos >= K ? pos - K : pos;
    return p;
}

// Forward recursion over n2 + 4 steps, two steps per round.  fetch() starts the loads of the next step pair's three soft values
// (type-4 bits at three consecutive interleaver positions) and returns what make(raw) needs to turn them into branch metrics;
// st(u, word) receives decision_word of steps 2u, 2u + 1.  The loads of pair u + 1 are issued BEFORE the add-compare-select of pair
// u and consumed after it (software pipelining by one round): a wavefront that has its SIMD to itself -- the last long blocks of a
// launch, every wave of a small one -- does not wait for LDS.  n2 is even for every block kind.  s0 = the start metric of state 0,
// 127 * N * K in the units of the branch metrics: 20 for classes in units of 127, 2540 for raw soft values (soft_core.hpp).
// probe(u, De, Do) sees the differences of steps 2u, 2u + 1 -- every pair, the flush steps included -- as acs_step left them: the list
// decoder (list_core.hpp) collects its margins there; the default sees nothing and costs nothing.
struct NoProbe { LM_MEM void operator()(int, const Pk*, const Pk*) const {} };
template <class Fetch, class Make, class St, class Probe = NoProbe>
LM_FN void viterbi_forward(int n2, Fetch fetch, Make make, St st, int s0 = 4 * 5, Probe probe = Probe()) {
    PathMetrics pm;
#pragma unroll
    for (int i = 0; i < 8; ++i) pm.R[i] = pk_make(0, 0);
    pm.R[0] = pk_make(s0, 0);
    auto raw = fetch();
    for (int u = 0; u < n2 / 2; ++u) {
        const Bm m = make(raw);
        if (u + 1 < n2 / 2) raw = fetch();
        Pk De[8], Do[8];
        const Pk Me[8] = { m.P, m.Q, m.Q, m.P, pk_swap(m.Q), pk_swap(m.P), pk_swap(m.P), pk_swap(m.Q) };
        acs_step(pm, Me, De);
        const Pk Mo[8] = { m.C, m.C, m.C, m.C, pk_swap(m.C), pk_swap(m.C), pk_swap(m.C), pk_swap(m.C) };
        acs_step(pm, Mo, Do);
        st(u, decision_word(De, Do));
        probe(u, De, Do);
    }
#pragma unroll
    for (int f = 0; f < kFlush / 2; ++f) {
        const Pk z = pk_make(0, 0);
        const Pk Mz[8] = { z, z, z, z, z, z, z, z };
        Pk De[8], Do[8];
        acs_step(pm, Mz, De);
        acs_step(pm, Mz, Do);
        st(n2 / 2 + f, decision_word(De, Do));
        probe(n2 / 2 + f, De, Do);
    }
}
// what fetch() hands to make(): the three LDS words that hold a step pair's soft values and where in them
struct Raw3 { uint32_t w[3]; uint32_t at[3]; };

// CRC16-CCITT (crc_simple.c:59-77, :103-106: x^16 + x^12 + x^5 + 1, start 0xffff, bits MSB first, good = 0x1d0f over type1 + 16
// bits).  The traceback meets the bits last to first, so it runs the register BACKWARDS from the good value and checks that it
// arrives at the start value: the shift register step is invertible (the polynomial's constant term is 1),
//     forward   fb = msb(r) ^ d;  r = (r << 1) ^ (fb ? 0x1021 : 0)            inverse   fb = r & 1;  r = ((r ^ fb * 0x1021) >> 1) | (fb ^ d) << 15
// and eight inverse steps are one table look-up: r = (r >> 8) ^ Tinv[r & 0xff] ^ (the eight bits, first one most significant, << 8)
// (the data bits enter at bit 15 and only shift right afterwards).  Until round 6 the CRC was folded in bit by bit (an AND + XOR with
// a position constant per bit, three instructions); this is five instructions and a look-up per eight bits.
// The register is carried shifted left by two (r4 = r << 2; whatever lands in its two low bits is never looked at) and the table
// holds Tinv << 2, so that r4 & 0x3fc is the byte offset of the table entry: one AND makes the LDS address.
struct CrcInvTable { uint32_t t[256]; };
constexpr uint32_t crc_inv_step(uint32_t r, uint32_t d) {
    const uint32_t fb = r & 1u;
    return ((r ^ (fb ? 0x1021u : 0u)) >> 1) | ((fb ^ d) << 15);
}
constexpr CrcInvTable make_crc_inv_table() {
    CrcInvTable c{};
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t r = b;
        for (int k = 0; k < 8; ++k) r = crc_inv_step(r, 0u);
        c.t[b] = r << 2;
    }
    return c;
}

// Traceback from state 0 after the flush steps with the CRC check run backwards alongside.  ld(u) returns the decision word of step
// pair u as the forward pass stored it; st(h, half) receives decoded bits 16h..16h+15 (bit 16h+b at bit b); tinv(off) = the entry of
// make_crc_inv_table at BYTE offset off (per-lane).  n2 = type1 + 16 CRC-covered bits + 4 tail bits, a multiple of 16.  Returns whether the CRC
// over the first n2 - 4 decoded bits is good.
// y = 15 - state runs in a shift register: the predecessor of state s under decision d is (2 s + d) & 15, so y' = 2 y + 1 - d, and
// the decision of state s sits at bit 2 y (odd step) or 2 y + 1 (even step) of the word: a shift, a one-bit signed extract (= -d)
// and an add per step.  The decoded bit of a step is the complement of bit 3 of y before the step, and the register only ever
// shifts, so after the 16 steps of group h bits 4..31 of ~y are the decoded bits 16h .. 16h+27: the CRC bytes, which end 4 bits
// before a group boundary, are cut from there -- bits 16h+12..16h+19 (not in the top group: tail bits) and 16h+4..16h+11; the four
// bits 0..3 left at the end take four single steps.
// flip(step) = all ones where the decision met at that step is to be inverted, else 0 (one XOR on the extracted -d): a candidate path
// of the list decoder (list_core.hpp); the default inverts nothing and costs nothing.
struct NoFlip { LM_MEM uint32_t operator()(int) const { return 0u; } };
template <class Ld, class St, class Tinv, class Flip = NoFlip>
LM_FN bool viterbi_traceback(int n2, Ld ld, St st, Tinv tinv, Flip flip = Flip()) {
    uint32_t y = 15u;
#pragma unroll
    for (int f = kFlush / 2 - 1; f >= 0; --f) {
        const uint32_t w = ld(n2 / 2 + f);
        uint32_t t = y << 1;
        y = t + 1u + (bfe_mask(w, t) ^ flip(n2 + 2 * f + 1));
        t = (y << 1) | 1u;
        y = t + (bfe_mask(w, t) ^ flip(n2 + 2 * f));
    }
    uint32_t r4 = kCrcOk << 2;
    const int top = n2 / 16 - 1;
    // the eight decision words of a group are requested one group ahead of their use (the scratch is in L2 / HBM: ~2000 clocks)
    uint32_t cur[8], nxt[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int b2 = 0; b2 < 8; ++b2) cur[b2] = ld(8 * top + b2);
    for (int h = top; h >= 0; --h) {
        if (h > 0) {
#pragma unroll
            for (int b2 = 0; b2 < 8; ++b2) nxt[b2] = ld(8 * (h - 1) + b2);
        }
#pragma unroll
        for (int b2 = 7; b2 >= 0; --b2) {
            const uint32_t w = cur[b2];
            uint32_t t = y << 1;
            y = t + 1u + (bfe_mask(w, t) ^ flip(16 * h + 2 * b2 + 1));
            t = (y << 1) | 1u;
            y = t + (bfe_mask(w, t) ^ flip(16 * h + 2 * b2));
        }
        const uint32_t bits = ~y;
        st(h, (bits >> 4) & 0xffffu);
        const uint32_t rev = rev32(bits);                 // decoded bit 16h + k at bit 27 - k
        if (h != top) r4 = (r4 >> 8) ^ tinv(r4 & 0x3fcu) ^ ((rev << 2) & 0x3fc00u);          // bits 16h+12 .. 16h+19
        r4 = (r4 >> 8) ^ tinv(r4 & 0x3fcu) ^ ((rev >> 6) & 0x3fc00u);                        // bits 16h+4 .. 16h+11
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2) cur[b2] = nxt[b2];
    }
    uint32_t r = (r4 >> 2) & 0xffffu;
#pragma unroll
    for (int k = 3; k >= 0; --k) r = crc_inv_step(r, (~y >> (4 + k)) & 1u);                         // bits 3 .. 0
    return r == 0xffffu;
}

// 4 decoded bits -> 4 bytes (one bit per byte, little endian)
LM_FN uint32_t spread4(uint32_t nib) { return (nib * 0x00204081u) & 0x01010101u; }

// Steps 2-3 for a lane whose type-4 bits (BITS: bit i at bit 31 - (i & 31) of word i >> 5) or soft classes (16 per word, descramble_chunk)
// are behind cls(word).  io = the lane's other memory: dec_st(u, word) / dec_ld(u) its decision word of step pair u, out_st(h, half)
// its decoded bits 16h .. 16h+15, tinv(off) the backward CRC table.  Returns the lane's CRC verdict.
template <class Io, class Flip = NoFlip>
LM_FN bool traceback(int type2, Io& io, Flip flip = Flip()) {        // (own lane's data only: program order is enough)
    return viterbi_traceback(type2, [&](int u) { return io.dec_ld(u); }, [&](int h, uint32_t half) { io.out_st(h, half); },
                             [&](uint32_t off) { return io.tinv(off); }, flip);
}
// step 2 alone: dec_st(u, word) as viterbi_forward's st, probe as there
template <bool BITS, class Cls, class DecSt, class Probe = NoProbe>
LM_FN void forward_hard(int type345, int type2, int a, Cls cls, DecSt dec_st, Probe probe = Probe()) {
    int pos = a;                       // (a * i) % K for i = 1
    auto fetch = [&] {
        Raw3 r;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int p = interleave_next(pos, a, type345);
            r.w[k] = cls(BITS ? p >> 5 : p >> 4);
            r.at[k] = BITS ? 31u - (uint32_t)(p & 31) : (uint32_t)(30 - 2 * (p & 15));
        }
        return r;
    };
    if (BITS) {
        viterbi_forward(type2, fetch,
                        [&](const Raw3& r) { return bm_from_masks(bfe_mask(r.w[0], r.at[0]), bfe_mask(r.w[1], r.at[1]), bfe_mask(r.w[2], r.at[2])); },
                        dec_st, 4 * 5, probe);
    } else {
        viterbi_forward(type2, fetch,
                        [&](const Raw3& r) { return bm_from_classes((int)(r.w[0] << r.at[0]) >> 30, (int)(r.w[1] << r.at[1]) >> 30, (int)(r.w[2] << r.at[2]) >> 30); },
                        dec_st, 4 * 5, probe);
    }
}
template <bool BITS, class Cls, class Io>
LM_FN bool decode_hard(int type345, int type2, int a, Cls cls, Io& io) {
    forward_hard<BITS>(type345, type2, a, cls, [&](int u, uint32_t w) { io.dec_st(u, w); });
    return traceback(type2, io);
}

// ---- channel bit errors of a decoded block (include/ext/tetra_biterr.h) ------------------------------------------------------------------
// The decoded type-2 bits d[0 .. type2) -- all of them, the four tail positions included -- are encoded again as a transmitter would
// (tetra_conv_enc.c:45-60 from the all-zero state, punct_2_3, tetra_interleave.c:36-39) and held against what was received: the
// Hamming distance from the received word to the decoded codeword over the positions that carry a decision.  The scrambler is a
// bijection on bits, so the comparison is made on the descrambled side, where the lane's staged data already is.
//   half(h)  = decoded bits 16h .. 16h+15, bit 16h + b at bit b (what viterbi_traceback hands to its st)
//   rx(p)    = type-4 position p as received: bit 0 = the position carries a decision, bit 1 = its hard bit
// Sixteen trellis steps at a time: with D = d[16h - 4 .. 16h + 15] (d[t] at bit t - 16h + 4, zeros before the block) the generators
// g1 = 1 + D + D^4 and g2 = 1 + D^2 + D^3 + D^4 of all sixteen steps are three and four shifted XORs.  Rate 2/3 sends g1 and g2 of
// every even step and g1 of every odd one (see the depuncturer above), in that order, and type-3 bit j sits at type-4 position
// (a (j + 1)) % K: the received bits are gathered with the decoder's running index into words that line up with g1 (every step) and
// g2 (even steps), and one XOR, AND and population count each give the group's share.  Returns errors | compared << 16.
template <class Half, class Rx>
LM_FN uint32_t reencode_errors(int type345, int type2, int a, Half half, Rx rx) {
    int pos = a;
    uint32_t prev = 0, errors = 0, compared = 0;
    for (int h = 0; h < type2 / 16; ++h) {
        const uint32_t D = ((uint32_t)half(h) << 4) | prev;
        prev = D >> 16;
        const uint32_t g1 = (D >> 4) ^ (D >> 3) ^ D, g2 = (D >> 4) ^ (D >> 2) ^ (D >> 1) ^ D;      // bit b: step 16h + b
        uint32_t r1 = 0, v1 = 0, r2 = 0, v2 = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t xa = rx(interleave_next(pos, a, type345));
            const uint32_t xb = rx(interleave_next(pos, a, type345));
            const uint32_t xc = rx(interleave_next(pos, a, type345));
            v1 |= ((xa & 1u) << (2 * u)) | ((xc & 1u) << (2 * u + 1));
            r1 |= ((xa >> 1) << (2 * u)) | ((xc >> 1) << (2 * u + 1));
            v2 |= (xb & 1u) << (2 * u);
            r2 |= (xb >> 1) << (2 * u);
        }
        errors += (uint32_t)__builtin_popcount((r1 ^ g1) & v1) + (uint32_t)__builtin_popcount((r2 ^ g2) & v2);
        compared += (uint32_t)__builtin_popcount(v1) + (uint32_t)__builtin_popcount(v2);
    }
    return errors | (compared << 16);
}
// ... for the hard routes: cls as decode_hard's.  A packed bit always carries a decision; a class is +1 (0b01: a 0), 0 (erasure) or -1
// (0b11: a 1), so its low bit says whether it counts and its high bit is the hard bit.
template <bool BITS, class Half, class Cls>
LM_FN uint32_t bit_errors_hard(int type345, int type2, int a, Half half, Cls cls) {
    return reencode_errors(type345, type2, a, half, [&](int p) -> uint32_t {
        return BITS ? 1u | (bfe_u(cls(p >> 5), 31u - (uint32_t)(p & 31), 1u) << 1) : bfe_u(cls(p >> 4), 2u * (uint32_t)(p & 15), 2u);
    });
}

// Step 4: the workgroup's decoded rows -> memory, the lane's share; half(h, q) = decoded bits 16h .. 16h+15 of row q.  WIDE (rows_wide):
// 8 bits -> 8 bytes per store, st8(q, d, v) = bytes 8d .. 8d+7 of row q, the (row, unit) index space flattened so that every lane
// stores in every round; otherwise st4(q, d, v) = bytes 4d .. 4d+3, row by row.
template <class Half, class St8, class St4>
LM_FN void write_rows(int lane, int rows_here, int type2, bool wide, Half half, St8 st8, St4 st4) {
    if (wide) {
        const int units = type2 >> 3, total = rows_here * units;
        const uint32_t inv = unit_inverse(units);
        for (int i = lane; i < total; i += kLanes) {
            const int q = unit_row(i, inv), d = i - q * units;
            const uint32_t byte = ((uint32_t)half(d >> 1, q) >> (8 * (d & 1))) & 0xffu;
            demux_core::U2 v;
            v.x = spread4(byte & 0xfu);
            v.y = spread4(byte >> 4);
            st8(q, d, v);
        }
    } else {
        const int out_dw = type2 >> 2;
        for (int q = 0; q < rows_here; ++q)
            for (int d = lane; d < out_dw; d += kLanes) st4(q, d, spread4(((uint32_t)half(d >> 2, q) >> (4 * (d & 3))) & 0xfu));
    }
}

// ---- SB1 tracking (tetra_lmac_track_*_device): the SYNC PDU, the scrambling code and the TDMA clock -------------------------------
// Host and device: tetra_lmac_scramb_init and the tracker kernel use the same source.
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define LM_HD __host__ __device__ __forceinline__
#else
#define LM_HD inline
#endif

// tetra_scramb.c:87-99: colour (6 bits) | MNC (14) << 6 | MCC (10) << 20, then two 1 bits shifted in below
LM_HD uint32_t scramb_code(uint32_t colour, uint32_t mcc, uint32_t mnc) {
    return (((colour & 0x3f) | ((mnc & 0x3fff) << 6) | ((mcc & 0x3ff) << 20)) << 2) | kScrambInitSb1;
}

// The fields tp_sap_udata_ind's SB1 case reads from a SYNC PDU (tetra_lower_mac.c:246-275), read from v = type-2 bits 0..55 of the
// SB1 block, bit 0 at bit 63.
struct SyncPdu {
    uint64_t v;
    LM_HD uint32_t field(int first, int len) const { return (uint32_t)(v >> (64 - first - len)) & ((1u << len) - 1u); }
    LM_HD uint32_t colour() const { return field(4, 6); }
    LM_HD uint32_t tn() const { return field(10, 2) + 1u; }          // as tcd->time holds it: the PDU's timeslot field + 1
    LM_HD uint32_t fn() const { return field(12, 5); }
    LM_HD uint32_t mn() const { return field(17, 6); }
    LM_HD uint32_t mcc() const { return field(31, 10); }
    LM_HD uint32_t mnc() const { return field(41, 14); }
};

// The PHY's TDMA clock (tetra_tdma.c:28-78).  One tetra_tdma_time_add_tn(t, 1), wrap thresholds to the letter: any state lands in
// tn 0..4, fn 0..18, mn 0..60.
struct Tdma { uint32_t tn, fn, mn; };
LM_HD void tdma_add_tn(Tdma& t) {
    t.tn += 1;
    if (t.tn > 4) { const uint32_t d = t.tn / 4; t.tn = t.tn % 4; t.fn += d; }
    if (t.fn > 18) { const uint32_t d = t.fn / 18; t.fn = t.fn % 18; t.mn += d; }
    if (t.mn > 60) t.mn = t.mn % 60;
}
// k >= 1 calls of tetra_tdma_time_add_tn(t, 1): one literal step, then k - 1 in closed form (from there on the three counters run
// 1..4, 1..18, 1..60, a zero taking one step to become 1)
LM_HD Tdma tdma_advance(Tdma t, uint32_t k) {
    tdma_add_tn(t);
    k -= 1;
    if (k) {
        const uint32_t p1 = t.tn + k - 1u;                                // t.tn in 0..4: a zero needs one step to become 1
        const uint32_t c1 = p1 >> 2;
        t.tn = (p1 & 3u) + 1u;
        if (c1) {
            const uint32_t p2 = t.fn + c1 - 1u, c2 = p2 / 18u;
            t.fn = p2 - 18u * c2 + 1u;
            if (c2) t.mn = (t.mn + c2 - 1u) % 60u + 1u;
        }
    }
    return t;
}
// the packed time of the tracker's outputs: tn | fn << 8 | mn << 16
LM_HD uint32_t tdma_pack(Tdma t) { return t.tn | (t.fn << 8) | (t.mn << 16); }

// ---- The SB1 tracking rule of one frame slot (k_track in tetra_lmac.hip; tests/emul/lmac_emul.cpp runs the same functions on the host) ----
// tp_sap_udata_ind (tetra_lower_mac.c) copies t_phy_state.time to tcd->time on entry of EVERY call (:172), overwrites its tn / fn / mn
// from a SYNC PDU only when the CRC is good (:257-266) and copies tcd->time back to t_phy_state.time for every SB1 (:268).  So:
//   every frame the LOCKED receiver consumes      t_phy_state.time += one timeslot (tetra_burst_sync.c:113, before the callback)
//   a SYNC burst's SB1 block, good CRC            tcd <- colour code, mcc, mnc, scramb_init; the clock <- the PDU's tn (bits + 1), fn, mn
//   a SYNC burst's SB1 block, bad CRC             the clock stays at its time on entry
// Slots are taken 64 at a time, a slot per lane.  What a slot needs from its past is the last SYNC frame with a GOOD CRC before it
// -- the clock was set there, and tcd holds that frame's fields -- and how many slots ago that was: the highest set bit below the
// lane in the group's mask of good frames; the fields come from that lane; the clock k slots later is tdma_advance.

// The tracker's state per channel: tetra_lmac_cell_state_t (include/tetra_lmac.h), member for member.
struct TrackState {
    uint32_t scramb_init, colour, mcc, mnc;
    Tdma tcd;        // tn / fn / mn of the last SYNC PDU with a good CRC (zero before the first)
    Tdma phy;        // t_phy_state.time
};
// What the rule gives for one slot.
struct TrackSlot {
    Tdma t_rx;       // t_phy_state.time on entry of tetra_burst_rx_cb
    Tdma t_after;    // ... after the slot's SB1 (every later block of the burst is handled under it; the next slot's step starts from it)
    Tdma tcd;        // the last good SYNC PDU's time up to and including this slot
    uint32_t colour, mcc, mnc, scramb;      // tcd's fields after the slot, the scrambling code in force for the slot's other blocks
};
// highest set bit of m at or below position `upto` (-1: none; upto = -1: none)
LM_FN int last_set_upto(unsigned long long m, int upto) {
    if (upto < 0) return -1;
    const unsigned long long x = m & (upto >= 63 ? ~0ull : ((2ull << upto) - 1ull));
    return x ? 63 - __builtin_clzll(x) : -1;
}
// The two words a lane keeps of a SYNC PDU with a good CRC: a = colour << 2 | tn << 8 | fn << 11 | mn << 16, b = mcc | mnc << 10.
// word(k) = bytes 4k .. 4k+3 of the decoded SB1 row (a bit per byte), little endian.
template <class Word>
LM_FN void sync_pdu_words(Word word, uint32_t& a, uint32_t& b) {
    uint64_t v = 0;                               // type-2 bits 0..55, first bit most significant
#pragma unroll
    for (int k = 0; k < 14; ++k) v |= (uint64_t)pack4(word(k) & 0x01010101u) << (60 - 4 * k);
    const SyncPdu p = { v };
    a = (p.colour() << 2) | (p.tn() << 8) | (p.fn() << 11) | (p.mn() << 16);
    b = p.mcc() | (p.mnc() << 10);
}
// st: the state the 64-slot group starts from.  mv / mg: the group's masks of slots that hold a SYNC burst / one with a good CRC (bit =
// lane).  words(h, a, b): the PDU words of lane h >= 0 (a lane shuffle on the device: every lane calls track_slot, none is masked off).
// kStaleTcdOnBadCrc = true is NOT the reference's rule: it is the rule this tracker had before it was pinned to the reference's own
// tp_sap_udata_ind -- an SB1 with a bad CRC throws the clock back to the time of the last good SYNC PDU -- kept so that the tests can
// plant it and show that they notice (tests/test_sync_track.py); nothing in the library instantiates it.
template <bool kStaleTcdOnBadCrc = false, class Words>
LM_FN TrackSlot track_slot(const TrackState& st, unsigned long long mv, unsigned long long mg, int lane, Words words) {
    // tcd as a slot sees it: the fields of good frame h, or what the group started with
    auto tcd_of = [&](int h, uint32_t ah, uint32_t bh, uint32_t& colour, uint32_t& mcc, uint32_t& mnc) {
        Tdma t = st.tcd;
        colour = st.colour; mcc = st.mcc; mnc = st.mnc;
        if (h >= 0) {
            t = Tdma{ (ah >> 8) & 7u, (ah >> 11) & 0x1fu, (ah >> 16) & 0x3fu };
            colour = (ah >> 2) & 0x3fu; mcc = bh & 0x3ffu; mnc = bh >> 10;
        }
        return t;
    };
    const int gp = last_set_upto(kStaleTcdOnBadCrc ? mv : mg, lane - 1);    // the last frame before this slot that set the clock
    const int hp = gp >= 0 ? last_set_upto(mg, gp) : -1;                    // ... and the good one whose time it took (gp itself)
    const int hs = last_set_upto(mg, lane);                                 // the good one tcd holds after this slot
    uint32_t ap, bp, as, bs;
    words(hp < 0 ? 0 : hp, ap, bp);
    words(hs < 0 ? 0 : hs, as, bs);
    TrackSlot o;
    // time on entry: k slots after the clock was last set, or after the group's start
    Tdma from = tcd_of(hp, ap, bp, o.colour, o.mcc, o.mnc);
    if (gp < 0) from = st.phy;
    o.t_rx = tdma_advance(from, (uint32_t)(lane - gp));
    // after the slot's SB1: the PDU's time if its CRC is good, else unchanged
    o.tcd = tcd_of(hs, as, bs, o.colour, o.mcc, o.mnc);
    const bool sets_clock = ((kStaleTcdOnBadCrc ? mv : mg) >> lane) & 1ull;
    o.t_after = sets_clock ? o.tcd : o.t_rx;
    o.scramb = st.scramb_init;                                              // (an if, not ?:, compiles the list form to the same code
    if (hs >= 0) o.scramb = scramb_code(o.colour, o.mcc, o.mnc);            //  as the formula written out in place)
    return o;
}
// The state after a group = after its last live slot (the next group, and the next call, start from it).
LM_FN void track_carry(TrackState& st, const TrackSlot& end) {
    st.phy = end.t_after;
    st.tcd = end.tcd;
    st.colour = end.colour; st.mcc = end.mcc; st.mnc = end.mnc;
    st.scramb_init = end.scramb;
}

// ---- AACH: the shortened (30,14) Reed-Muller code of EN 300 392-2 8.2.3.2 (include/tetra_aach.h) ----------------------------------------
// A word holds the block's 30 bits, first bit on air at bit 29: the 14 information bits in bits 29..16, the 16 parity bits in bits
// 15..0 -- the value format of the reference's tetra_rm3014_compute (lower_mac/tetra_rm3014.c), whose decoder is a stub ("Maybe
// correct it in the future") and whose caller (tetra_lower_mac.c:230-236, "FIXME: RM3014-decode") never calls it.  The code is
// systematic, G = [I | P]; row i of P (the parity bits information bit i sets, i = 0 the first bit on air) is a constant of the
// standard like the training sequences.  Minimum distance 8: the 4526 error patterns of weight <= 3 have 4526 distinct syndromes, so
// up to three bit errors are corrected and every fourth is detected (tests/test_aach_rm.py checks both exhaustively).
constexpr int kRm3014Radius = 3;
constexpr uint32_t kRm3014Undecodable = 0xffu;            // `dist` of a word no codeword lies within the radius of
constexpr uint32_t kRm3014TableEntries = 1u << 16;        // one per syndrome: 256 KB
constexpr uint32_t kRm3014NoPattern = 0xffffffffu;        // table entry of a syndrome no pattern of weight <= 3 has
// the 16 parity bits of 14 information bits (first bit at bit 13): 14 x (extract, AND, XOR) on constants
LM_HD uint32_t rm3014_parity(uint32_t info) {
    constexpr uint32_t rows[14] = { 0x9b60u, 0x2de0u, 0xfc20u, 0xe03cu, 0x983au, 0x5436u, 0x2c2eu,
                                    0xffdfu, 0x8339u, 0x42b5u, 0x21adu, 0x1273u, 0x096bu, 0x04e7u };
    uint32_t p = 0;
#pragma unroll
    for (int i = 0; i < 14; ++i) p ^= rows[i] & (0u - ((info >> (13 - i)) & 1u));
    return p;
}
LM_HD uint32_t rm3014_encode(uint32_t info) { return ((info & 0x3fffu) << 16) | rm3014_parity(info & 0x3fffu); }
// H w for H = [P^T | I]: zero exactly for codewords, and the syndrome of (codeword ^ e) is that of e
LM_HD uint32_t rm3014_syndrome(uint32_t word) { return rm3014_parity((word >> 16) & 0x3fffu) ^ (word & 0xffffu); }
// Syndrome -> the one error pattern of weight <= 3 that has it (kRm3014NoPattern where there is none), from the generator alone:
// host code, run once per device (tetra_lmac.hip) and by the host emulation.
inline void rm3014_correction_table(uint32_t* tab) {      // [kRm3014TableEntries]
    for (uint32_t s = 0; s < kRm3014TableEntries; ++s) tab[s] = kRm3014NoPattern;
    tab[0] = 0;
    for (int a = 0; a < 30; ++a) {
        const uint32_t ea = 1u << a;
        tab[rm3014_syndrome(ea)] = ea;
        for (int b = a + 1; b < 30; ++b) {
            const uint32_t eb = ea | (1u << b);
            tab[rm3014_syndrome(eb)] = eb;
            for (int c = b + 1; c < 30; ++c) tab[rm3014_syndrome(eb | (1u << c))] = eb | (1u << c);
        }
    }
}
// Bounded-distance decoding with radius 3: the codeword within Hamming distance <= 3 of `word` (unique: d = 8) and that distance,
// else the word unchanged and kRm3014Undecodable.  tab(s) = entry s of rm3014_correction_table; one look-up, no search.
struct Rm3014Word { uint32_t word, dist; };
template <class Tab>
LM_HD Rm3014Word rm3014_decode(uint32_t word, Tab tab) {
    word &= 0x3fffffffu;
    const uint32_t e = tab(rm3014_syndrome(word));
    const bool found = (e >> 30) == 0u;
    return Rm3014Word{ found ? word ^ e : word, found ? (uint32_t)__builtin_popcount(e) : kRm3014Undecodable };
}

}  // namespace tetra_lmac
