// soft_core.hpp -- lane-level code of the receive chain's soft-decision option (TETRA_RX_FLAG_SOFT, include/tetra_rx.h): the
// quantiser behind the demodulator (k_soft in tetra_rx.hip) and the soft front end + forward recursion of the frame decoder
// (k_lmac_frames_soft in tetra_lmac.hip).  Compiled by hipcc for gfx950 and by g++ (-DTETRA_HOST_EMUL) into
// tests/emul/lmac_soft_emul.cpp, which holds it bit for bit against the reference's conv_cch_decode (viterbi_cch.c -> osmo_conv.c).
//
// Soft value of a bit.  With s[k] the demodulator's post-Costas symbol k of a channel and d = s[k] * conj(s[k-1]) (separate
// binary32 multiplies and adds, no contraction), the differential phases 0, pi/2, pi, -pi/2 carry the dibits 00, 01, 11, 10
// (dqpsk_sym_extr.cpp:32-51), so
//     bit 2k   (first of the dibit):   v = d.re + d.im
//     bit 2k+1 (second):               v = d.re - d.im
// positive = bit 0, the reference's sbit convention (viterbi.c:11-23).  A fresh channel's previous symbol is (1,1)/sqrt(2): the
// slicer's prev = 0 (quadrant 0).
//
// Quantisation.  q = clamp(rintf(G * v), -Q, Q), NaN -> 0, +-Inf -> +-Q, with
//     G = 16      the demodulator's AGC holds |s|^2 near 1, so a clean bit sits at +-16, half of full scale: noise on top of a
//                 good symbol is not clipped, and a clean bit is 16 quantiser steps from its decision threshold;
//     Q = 31      six bits.
// Why Q = 31 is safe.  Per step pair (one even, one odd trellis step; rate 2/3: three soft values) a path metric moves by at
// most |sa + sb| + |sc| <= 3 Q, the flush steps add nothing, and the start metric of state 0 is the reference's 127 * N * K = 2540
// in raw units (osmo_conv.c:528) where the hard route has 20 units of 127.  Over the longest block's 144 pairs every metric stays
// inside [-432 Q, 2540 + 432 Q] = [-13392, 15932]; an add-compare-select forms sums one branch metric (<= 2 Q) outside that and
// their difference, |D| <= 2540 + 864 Q + 4 Q = 29448 < 32767: the packed int16 lanes of lmac_core.hpp need no renormalisation.
// The reference's own sums are int16 too, never above 2540 + 292 * 2 Q = 20644 and renormalised to a minimum of 0 every 59 steps
// (osmo_conv.c:137-153, :642), so it does not overflow on these values either and both make the same decisions.
#pragma once

#include <math.h>
#include <stdint.h>

#include "lmac_core.hpp"

namespace tetra_soft {

using namespace tetra_lmac;

constexpr int kQ = 31;
constexpr float kG = 16.0f;
constexpr int kStartMetric = 127 * 4 * 5;         // osmo_conv.c:528 in raw units
constexpr float kFreshPrev = 0.70710678f;       // both components of a fresh channel's previous symbol

LM_FN int quantise(float v) {
    float x = kG * v;
    x = x < -(float)kQ ? -(float)kQ : x;
    x = x > (float)kQ ? (float)kQ : x;          // (a NaN fails both comparisons)
    return x != x ? 0 : (int)rintf(x);
}
// the two soft bits of symbol (sr, si) after (pr, pi)
LM_FN void soft_pair(float sr, float si, float pr, float pi, int& q0, int& q1) {
    const float a = sr * pr, b = si * pi, c = si * pr, d = sr * pi;
    const float re = a + b, im = c - d;
    q0 = quantise(re + im);
    q1 = quantise(re - im);
}

// ---- the ring ---------------------------------------------------------------------------------------------------------------------
// One int8 per bit, per channel, at (absolute bit number) mod R: the numbering of the burst synchroniser (tetra_rx_block_t.bitnum).
// The tail of call k reads bits of the frames the synchroniser consumed in call k: they lie in its 4096-bit buffer or among the
// call's new bits, [n_k - 4096, n_k + b_k) with n_k the bit count before the call and b_k <= stride the call's bits.  With two
// calls in flight the quantiser of call k + 1 writes [n_k + b_k, n_k + b_k + b_{k+1}) meanwhile (that of call k + 2 waits for tail k
// like the demodulator in front of it).  Both ranges together span at most 4096 + 2 stride bits, so they never meet in a ring of
//     R = the power of two >= 4096 + 2 stride                                   (at least 8192)
inline uint32_t ring_size(int bits_stride) {
    uint32_t r = 8192;
    while (r < 4096u + 2u * (uint32_t)bits_stride) r <<= 1;
    return r;
}

// ---- the decoder's front end --------------------------------------------------------------------------------------------------------
// The lane's block as biased bytes (soft value + 128) in type-4 order, four per word, descrambled by sign.
constexpr int kSoftWords = kMaxType345 / 4;            // 108 words = 432 bytes per lane

// bit 3 - b of a nibble -> 0xff in byte b (the nibble's first bit is its most significant, byte 0 the first soft value)
LM_FN uint32_t nibble_mask(uint32_t nib) { return (((nib * 0x01008040u) & 0x01010100u) | (nib >> 3)) * 0xffu; }
// Four soft values (signed bytes, |x| <= Q) -> biased, negated where `neg` has 0xff.  Biased y = x + 128 = x ^ 0x80; the negative is
// 128 - x = (255 - y) + 1, and 255 - y <= 255 - (128 - Q) leaves room for the + 1: no carry crosses a byte.
LM_FN uint32_t bias_and_flip(uint32_t four, uint32_t neg) { return ((four ^ 0x80808080u) ^ neg) + (neg & 0x01010101u); }
// four consecutive ring bytes from position a on; ring(w) = aligned word w of the channel's ring (R / 4 words, R = mask + 1)
template <class Ring>
LM_FN uint32_t ring_four(Ring ring, uint32_t a, uint32_t mask) {
    const uint32_t lo = ring((a & mask) >> 2), hi = ring(((a + 4u) & mask) >> 2);
    const uint32_t sh = 8u * (a & 3u);
    return sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
}
// The type-5 bits of a block = burst bits [off0, off0 + len0) then [off1, off1 + len1) of the frame that starts at absolute bit
// `bitnum`; seq = the lane's scrambling sequence (bit i at bit 31 - (i & 31) of word i >> 5); st(g, word) receives soft values
// 4g .. 4g+3.  Every piece of a coded kind is a multiple of four bits long, so no word straddles two pieces.
template <int TRAIN, int TPSAP, int BLK, class Ring, class St>
LM_FN void stage_pieces(uint32_t bitnum, bool present, Ring ring, uint32_t mask, const uint32_t seq[kSeqWords], St st) {
    const demux_core::Pieces p = demux_core::pieces_for(TRAIN, TPSAP, BLK);      // (literals after inlining, as in lmac_core's cut)
#pragma unroll
    for (int g = 0; g < (p.len0 + p.len1) / 4; ++g) {
        const int at = 4 * g < p.len0 ? p.off0 + 4 * g : p.off1 + 4 * g - p.len0;
        const uint32_t four = present ? ring_four(ring, bitnum + (uint32_t)at, mask) : 0u;     // a frame of another burst type: erasures
        st(g, bias_and_flip(four, nibble_mask((seq[g >> 3] >> (28 - 4 * (g & 7))) & 0xfu)));
    }
}
// the same literal layouts as frame_block (lmac_core.hpp)
template <class Ring, class St>
LM_FN void stage_block(int layout, uint32_t bitnum, int frame_type, Ring ring, uint32_t mask, const uint32_t seq[kSeqWords], St st) {
    switch (layout) {
        case kLayoutSb1: stage_pieces<TETRA_TRAIN_SYNC, TETRA_TPSAP_T_SB1, 1>(bitnum, frame_type == TETRA_TRAIN_SYNC, ring, mask, seq, st); break;
        case kLayoutSb2: stage_pieces<TETRA_TRAIN_SYNC, TETRA_TPSAP_T_SB2, 2>(bitnum, frame_type == TETRA_TRAIN_SYNC, ring, mask, seq, st); break;
        case kLayoutNdb1: stage_pieces<TETRA_TRAIN_NORM_2, TETRA_TPSAP_T_NDB, 1>(bitnum, frame_type == TETRA_TRAIN_NORM_2, ring, mask, seq, st); break;
        case kLayoutNdb2: stage_pieces<TETRA_TRAIN_NORM_2, TETRA_TPSAP_T_NDB, 2>(bitnum, frame_type == TETRA_TRAIN_NORM_2, ring, mask, seq, st); break;
        case kLayoutSchF: stage_pieces<TETRA_TRAIN_NORM_1, TETRA_TPSAP_T_SCH_F, 0>(bitnum, frame_type == TETRA_TRAIN_NORM_1, ring, mask, seq, st); break;
        default: break;
    }
}
// The soft front end (beside lmac_core.hpp's, one per source): the lane's sequence, then the block staged from its channel's ring.
// J: as frame_hard_block's; bitnum(), frame_type(): the frame's absolute bit number and burst type (accessors: loaded behind the
// sequence, where they are used); rows: as lane_sequence's; ring: as ring_four's, of ring_words words (R / 4); st as stage_block's.
template <class Job, class Bitnum, class FrameType, class Rows, class Ring, class St>
LM_FN void soft_block(const Job* J, uint32_t code, Bitnum bitnum, FrameType frame_type, Rows rows, Ring ring, uint32_t ring_words, St st) {
    uint32_t seq[kSeqWords] = {};
    lane_sequence(J->type345, code, rows, [&](int w, uint32_t word) { seq[w] = word; });
    stage_block(J->layout, bitnum(), frame_type(), ring, 4u * ring_words - 1u, seq, st);
}

// The forward recursion on the staged block: ld(w) = the lane's staged word w.  Deinterleaving and depuncturing are by address as
// on the hard routes (a punctured position never enters a branch metric: it is the reference's 0); dec_st as viterbi_forward's st.
// probe: as viterbi_forward's.
template <class Ld, class DecSt, class Probe = NoProbe>
LM_FN void forward(int type345, int type2, int a, Ld ld, DecSt dec_st, Probe probe = Probe()) {
    int pos = a;
    viterbi_forward(type2,
                    [&] {
                        Raw3 r;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const int p = interleave_next(pos, a, type345);
                            r.w[k] = ld(p >> 2);
                            r.at[k] = 8u * (uint32_t)(p & 3);
                        }
                        return r;
                    },
                    [&](const Raw3& r) {
                        return bm_from_classes((int)bfe_u(r.w[0], r.at[0], 8) - 128, (int)bfe_u(r.w[1], r.at[1], 8) - 128, (int)bfe_u(r.w[2], r.at[2], 8) - 128);
                    },
                    dec_st, kStartMetric, probe);
}
// steps 2-3 of the soft route: the forward recursion above, then the hard route's traceback (io: as decode_hard's)
template <class Ld, class Io>
LM_FN bool decode_soft(int type345, int type2, int a, Ld ld, Io& io) {
    forward(type345, type2, a, ld, [&](int u, uint32_t w) { io.dec_st(u, w); });
    return traceback(type2, io);
}

// reencode_errors (lmac_core.hpp) on the staged block: a soft value of zero carries no decision, a negative one is a 1.  half: as
// there; ld: as decode_soft's.
template <class Half, class Ld>
LM_FN uint32_t bit_errors_soft(int type345, int type2, int a, Half half, Ld ld) {
    return reencode_errors(type345, type2, a, half, [&](int p) -> uint32_t {
        const uint32_t y = bfe_u(ld(p >> 2), 8u * (uint32_t)(p & 3), 8);      // soft value + 128
        return (y != 128u ? 1u : 0u) | (y < 128u ? 2u : 0u);
    });
}

// ---- the AACH from soft values: exact maximum-likelihood decoding over the RM(30,14) code's 16384 codewords (ext/tetra_aach_soft.h) ------
// A staged AACH row is 32 plain signed bytes in 8 words: the block's 30 soft values descrambled by sign, then two zeros.  The search
// itself (k_aach_soft in tetra_lmac.hip) is a dense int8 product on the matrix cores; what it shares with the host emulation is here:
// the staging, the key that carries the tie rule, the running best two, and the read-out.
constexpr int kAachWords = 8;
constexpr int kAachMaxMargin = 930;                    // 30 values of magnitude Q: |corr| <= 930, and so is the margin

// four plain signed bytes (|x| <= Q), negated where `neg` has 0xff
LM_FN uint32_t flip_signed(uint32_t four, uint32_t neg) { return bias_and_flip(four, neg) ^ 0x80808080u; }
// The AACH's bits of a TRAIN burst (demux_core::pieces_for: SYNC one piece, the normal bursts 14 + 16) from the ring.  The pieces are no
// multiples of four, so a word may take its first bytes from the end of piece 0 and the rest from the start of piece 1: two reads, the
// second placed so that its bytes fall into the same byte lanes.  seq: the scrambling sequence's first word (bit i at bit 31 - i).
template <int TRAIN, class Ring>
LM_FN void stage_aach_pieces(uint32_t bitnum, Ring ring, uint32_t mask, uint32_t seq, uint32_t y[kAachWords]) {
    const demux_core::Pieces p = demux_core::pieces_for(TRAIN, TETRA_TPSAP_T_BBK, 0);
#pragma unroll
    for (int g = 0; g < kAachWords; ++g) {
        const int i = 4 * g;
        uint32_t four;
        if (i + 4 <= p.len0 || p.len1 == 0) four = ring_four(ring, bitnum + (uint32_t)(p.off0 + i), mask);
        else if (i >= p.len0) four = ring_four(ring, bitnum + (uint32_t)(p.off1 + i - p.len0), mask);
        else {
            const uint32_t first = 0xffffffffu >> (8 * (4 - (p.len0 - i)));          // the bytes piece 0 still has
            four = (ring_four(ring, bitnum + (uint32_t)(p.off0 + i), mask) & first) | (ring_four(ring, bitnum + (uint32_t)(p.off1 + i - p.len0), mask) & ~first);
        }
        y[g] = flip_signed(four, nibble_mask((seq >> (28 - 4 * g)) & 0xfu));
    }
    y[kAachWords - 1] &= 0x0000ffffu;                  // values 30, 31: not the block's
}
// The AACH front end on soft values: the frame's 30 ring positions descrambled by sign with `code`; a frame of another burst type is 30
// erasures.  bitnum(), frame_type(), rows, ring, ring_words: as soft_block's.
template <class Bitnum, class FrameType, class Rows, class Ring>
LM_FN void aach_soft_block(uint32_t code, Bitnum bitnum, FrameType frame_type, Rows rows, Ring ring, uint32_t ring_words, uint32_t y[kAachWords]) {
    uint32_t seq = 0;
    lane_sequence(30, code, rows, [&](int w, uint32_t word) { seq = w == 0 ? word : seq; });
    const uint32_t bn = bitnum(), mask = 4u * ring_words - 1u;
    const int ft = frame_type();
#pragma unroll
    for (int g = 0; g < kAachWords; ++g) y[g] = 0u;
    if (ft == TETRA_TRAIN_SYNC) stage_aach_pieces<TETRA_TRAIN_SYNC>(bn, ring, mask, seq, y);
    else if (ft == TETRA_TRAIN_NORM_1 || ft == TETRA_TRAIN_NORM_2) stage_aach_pieces<TETRA_TRAIN_NORM_1>(bn, ring, mask, seq, y);
}
// soft value k of a staged row
LM_FN int aach_value(const uint32_t y[kAachWords], int k) { return (int)(int8_t)(y[k >> 2] >> (8 * (k & 3))); }

// corr and info in one int32 that orders codewords as the definition does: larger corr first, then the smaller info (|corr| <= 930)
LM_FN int aach_key(int corr, uint32_t info) { return corr * 16384 + (int)(16383u - info); }
// the two largest keys seen (best >= second): the new second is the median of (best, second, key)
struct Top2 { int best, second; };
constexpr int kTop2None = -0x7fffffff - 1;
LM_FN void top2_insert(Top2& t, int key) {
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
    int m;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(m) : "v"(t.best), "v"(t.second), "v"(key));
    t.second = m;
#else
    const int lo = t.best < key ? t.best : key;
    t.second = t.second > lo ? t.second : lo;
#endif
    t.best = t.best > key ? t.best : key;
}
// The read-out: best's information bits and codeword (word format of lmac_core.hpp's rm3014_encode), the margin to the runner-up
// (0 = a tie) and the number of non-zero values whose sign disagrees with best.
struct AachSoft { uint32_t info, word, dist, margin; };
LM_FN AachSoft aach_soft_finish(const Top2& t, const uint32_t y[kAachWords]) {
    AachSoft r;
    r.info = 16383u - ((uint32_t)t.best & 16383u);
    r.margin = (uint32_t)((t.best >> 14) - (t.second >> 14)) >> 1;
    r.word = rm3014_encode(r.info);
    uint32_t neg = 0, nz = 0;                           // value k at bit 29 - k, as the codeword's bits
#pragma unroll
    for (int k = 0; k < 30; ++k) {
        const int v = aach_value(y, k);
        neg |= (v < 0 ? 1u : 0u) << (29 - k);
        nz |= (v != 0 ? 1u : 0u) << (29 - k);
    }
    r.dist = (uint32_t)__builtin_popcount((neg ^ r.word) & nz);
    return r;
}
// bytes 30 and 31 of a row (dist, the margin saturated at a byte) as the top half of its last word, and the verdict
LM_FN uint32_t aach_soft_tail(const AachSoft& r) { return (r.dist << 16) | ((r.margin < 255u ? r.margin : 255u) << 24); }
LM_FN bool aach_soft_good(const AachSoft& r, int min_margin) { return (int)r.margin >= (min_margin < 1 ? 1 : min_margin); }

}  // namespace tetra_soft
