// tch_core.hpp -- lane-level code of the circuit-mode data channels TCH/7.2, TCH/4.8 and TCH/2.4 (include/ext/tetra_tch.h).
//
// A sibling of lmac_core.hpp, compiled twice like it: by hipcc into the kernels of tetra_lmac.hip and by g++ (-DTETRA_HOST_EMUL) into
// tests/emul/lmac_tch_emul.cpp.  What it shares with the signalling kinds is taken from there and not restated: the scrambler and the
// block front ends (a TCH block has the 432 type-5 bits and the (432, 103) interleaver of SCH/F), the packed path metrics and
// acs_step, decision_word, the traceback's shift-register step.  What is its own:
//   * the schedule    tetra_conv_enc.c:120-128, :148-164 restated.  Both puncturers walk the mother code in periods of 8 bits = one
//                     step PAIR and skip a type-3 index now and then: i = j + (j - 1) / 65 (TCH/4.8, P = {1, 2, 5} of 8: g1 g2 of the
//                     even step, g1 of the odd one) never reaches i = 66 m, the third value of pair 22 m - 1; i = j + (j - 1) / 35
//                     (TCH/2.4, P = {1, 2, 3, 5, 6, 7}: g1 g2 g3 of both steps) never reaches i = 36 m, the sixth value of pair 6 m - 1.
//                     So a pair carries 3 (6) values at consecutive type-3 indices, and every 22nd (6th) pair lacks its last one:
//                       TCH/4.8   1100 x 146, 1000 x 140, 0000 x 6        TCH/2.4   1110 x 136, 1100 x 12
//                     That closed form (pair u is short iff (u + 1) % period == 0) is all the kernels know of the puncturer.
//   * branch metrics  from g1, g2 and g3.  Butterfly i = (d0 d1 d2): g1 = d0, g2 = d1 ^ d2, g3 = d0 ^ d1 (g4 is never sent), so with
//                     the three soft classes sa, sb, sg:  m_0..3 = sa+sb+sg, sa-sb+sg, sa-sb-sg, sa+sb-sg  and  m_4..7 = -m_1, -m_0,
//                     -m_3, -m_2.  A generator a step does not carry is a constant zero and folds away.
//   * the traceback   from state 0 after the four flush steps, no CRC, for n2 = 292 and 148 = 16 H + 4: the top four bits first.
//   * bit errors      reencode_errors for three generators and the schedule above.
// Path metrics: classes in units of 127 and s0 = 20 as in lmac_core.hpp; 296 steps of at most +-3 stay far inside int16, and the
// reference's renormalisation (every 59 steps, 59 * 3 * 127 + 2540 < 32768) never changes a comparison.
#pragma once

#include "lmac_core.hpp"

namespace tetra_tch {

using namespace tetra_lmac;

// TETRA_LMAC_T_TCH_* (include/ext/tetra_tch.h)
enum { kTch72 = 8, kTch48 = 9, kTch24 = 10 };
constexpr int kType345 = 432;
constexpr int kInterleaveA = 103;
constexpr int kMaxType2 = 292;                            // of the coded kinds
constexpr int kOutHalves = (kMaxType2 + 15) / 16;         // 19
constexpr int kMaxPairs = (kMaxType2 + kFlush) / 2;       // 148

// ng: generators per step (0: not coded); a pair carries `vals` values and every `period`-th pair lacks its last one
struct Kind { int type2, type1, ng, vals, period; };
constexpr bool is_tch(int type) { return type >= kTch72 && type <= kTch24; }
constexpr Kind kind_of(int type) {
    return type == kTch48 ? Kind{ 292, 288, 2, 3, 22 } : type == kTch24 ? Kind{ 148, 144, 3, 6, 6 } : Kind{ 432, 432, 0, 0, 0 };
}
// the frame decoder's job table carries a block's type2 (DevJob): the generators per step of the TCH kind with that many type-2 bits
constexpr int ng_of_type2(int type2) { return type2 == 292 ? 2 : type2 == 148 ? 3 : 0; }
// the 2 x 4 pattern bits of step pair u (g1 g2 g3 g4 of the even step, then of the odd one, first at bit 7): the schedule as the
// tests hold it against tetra_rcpc_depunct
constexpr uint32_t pair_pattern(int ng, int u) {
    const bool is_short = ng == 2 ? (u + 1) % 22 == 0 : (u + 1) % 6 == 0;
    return ng == 2 ? (is_short ? 0xc0u : 0xc8u) : (is_short ? 0xecu : 0xeeu);
}

// the values of a step pair as the forward recursion fetches them: LDS words and where in them; keep = 0 where the last one is absent
template <int VALS> struct RawPair { uint32_t w[VALS]; uint32_t at[VALS]; uint32_t keep; };

// What a lane's descrambled block is made of: soft classes (2 bits, 16 per word), packed bits (32 per word), or the staged bytes of
// soft_core.hpp (soft value + 128, four per word: tch_soft_core.hpp).  kSrcClasses / kSrcBits are the BITS = false / true of decode_lane.
enum { kSrcClasses = 0, kSrcBits = 1, kSrcSoft = 2 };
template <int SRC> LM_FN uint32_t src_word(int p) { return (uint32_t)(SRC == kSrcBits ? p >> 5 : SRC == kSrcSoft ? p >> 2 : p >> 4); }
template <int SRC> LM_FN uint32_t src_at(int p) {
    return SRC == kSrcBits ? 31u - (uint32_t)(p & 31) : SRC == kSrcSoft ? 8u * (uint32_t)(p & 3) : (uint32_t)(30 - 2 * (p & 15));
}

// (s, -s) of the value k of a fetched pair: from a packed bit (0 -> +1, 1 -> -1), a 2-bit signed class or a staged byte (raw soft value)
template <int SRC, int VALS>
LM_FN Pk pair_value(const RawPair<VALS>& r, int k) {
    Pk v;
    if (SRC == kSrcBits) v = pk_from_bits(0xffff0001u ^ (bfe_mask(r.w[k], r.at[k]) & 0xfffefffeu));
    else if (SRC == kSrcSoft) {
        const int c = (int)bfe_u(r.w[k], r.at[k], 8) - 128;
        v = pk_make(c, -c);
    } else {
        const int c = (int)(r.w[k] << r.at[k]) >> 30;
        v = pk_make(c, -c);
    }
    return k == VALS - 1 ? pk_from_bits(pk_bits(v) & r.keep) : v;
}
// Mm[i] = (m_i, -m_i) of acs_step from the step's three values
LM_FN void step_metrics(Pk A, Pk B, Pk G, Pk Mm[8]) {
    const Pk X = pk_add(A, G), Y = pk_sub(A, G);
    const Pk M0 = pk_add(X, B), M1 = pk_sub(X, B), M2 = pk_sub(Y, B), M3 = pk_add(Y, B);
    Mm[0] = M0; Mm[1] = M1; Mm[2] = M2; Mm[3] = M3;
    Mm[4] = pk_swap(M1); Mm[5] = pk_swap(M0); Mm[6] = pk_swap(M3); Mm[7] = pk_swap(M2);
}

// Forward recursion over n2 + 4 steps, two per round, software-pipelined by one round like viterbi_forward.  cls(word): the lane's
// descrambled block (kSrcBits: bit i at bit 31 - (i & 31) of word i >> 5; kSrcClasses: soft classes, 16 per word; kSrcSoft: staged
// bytes, four per word); st(u, word): decision_word of steps 2u, 2u + 1; s0: the start metric of state 0 in the values' units, as
// viterbi_forward's.  The schedule runs as a countdown to the next short pair: wave-uniform, no division.
template <int NG, int SRC, class Cls, class St>
LM_FN void forward(int n2, Cls cls, St st, int s0 = 4 * 5) {
    constexpr int VALS = NG == 2 ? 3 : 6, PERIOD = NG == 2 ? 22 : 6;
    int pos = kInterleaveA, left = PERIOD;
    auto fetch = [&] {
        RawPair<VALS> r;
        const bool is_short = --left == 0;
        left = is_short ? PERIOD : left;
        r.keep = is_short ? 0u : 0xffffffffu;
#pragma unroll
        for (int k = 0; k < VALS; ++k) {
            int p = pos;
            if (k < VALS - 1 || !is_short) p = interleave_next(pos, kInterleaveA, kType345);      // (an absent value reads a live word and is masked)
            r.w[k] = cls((int)src_word<SRC>(p));
            r.at[k] = src_at<SRC>(p);
        }
        return r;
    };
    PathMetrics pm;
#pragma unroll
    for (int i = 0; i < 8; ++i) pm.R[i] = pk_make(0, 0);
    pm.R[0] = pk_make(s0, 0);
    const Pk z = pk_make(0, 0);
    auto raw = fetch();
    for (int u = 0; u < n2 / 2; ++u) {
        Pk Me[8], Mo[8], De[8], Do[8];
        if (NG == 2) {
            step_metrics(pair_value<SRC>(raw, 0), pair_value<SRC>(raw, 1), z, Me);
            step_metrics(pair_value<SRC>(raw, 2), z, z, Mo);
        } else {
            step_metrics(pair_value<SRC>(raw, 0), pair_value<SRC>(raw, 1), pair_value<SRC>(raw, 2), Me);
            step_metrics(pair_value<SRC>(raw, 3), pair_value<SRC>(raw, 4), pair_value<SRC>(raw, VALS - 1), Mo);
        }
        if (u + 1 < n2 / 2) raw = fetch();
        acs_step(pm, Me, De);
        acs_step(pm, Mo, Do);
        st(u, decision_word(De, Do));
    }
#pragma unroll
    for (int f = 0; f < kFlush / 2; ++f) {
        const Pk Mz[8] = { z, z, z, z, z, z, z, z };
        Pk De[8], Do[8];
        acs_step(pm, Mz, De);
        acs_step(pm, Mz, Do);
        st(n2 / 2 + f, decision_word(De, Do));
    }
}

// Traceback from state 0 behind the flush steps; ld(u): the decision word of step pair u, st(h, half): decoded bits 16h .. 16h+15 (bit
// 16h + b at bit b; the top group holds n2 % 16 bits, zeros above).  The step is viterbi_traceback's: y = 15 - state in a shift register,
// after the steps of group h bits 4.. of ~y are the decoded bits 16h ..; eight decision words are requested a group ahead of their use.
template <class Ld, class St>
LM_FN void traceback(int n2, Ld ld, St st) {
    uint32_t y = 15u;
    auto pair = [&](uint32_t w) {
        uint32_t t = y << 1;
        y = t + 1u + bfe_mask(w, t);
        t = (y << 1) | 1u;
        y = t + bfe_mask(w, t);
    };
#pragma unroll
    for (int f = kFlush / 2 - 1; f >= 0; --f) pair(ld(n2 / 2 + f));
    const int full = n2 >> 4, rest = (n2 & 15) >> 1;          // whole groups, step pairs above them
    for (int b2 = rest - 1; b2 >= 0; --b2) pair(ld(8 * full + b2));
    if (rest) st(full, (~y >> 4) & ((1u << (2 * rest)) - 1u));
    uint32_t cur[8], nxt[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int b2 = 0; b2 < 8; ++b2) cur[b2] = ld(8 * (full - 1) + b2);
    for (int h = full - 1; h >= 0; --h) {
        if (h > 0) {
#pragma unroll
            for (int b2 = 0; b2 < 8; ++b2) nxt[b2] = ld(8 * (h - 1) + b2);
        }
#pragma unroll
        for (int b2 = 7; b2 >= 0; --b2) pair(cur[b2]);
        st(h, (~y >> 4) & 0xffffu);
#pragma unroll
        for (int b2 = 0; b2 < 8; ++b2) cur[b2] = nxt[b2];
    }
}

// Channel bit errors of a decoded block (tetra_tch.h): reencode_errors of lmac_core.hpp for three generators and the schedule above.
// half(h) as traceback's st; rx(p) = type-4 position p as received: bit 0 = it carries a decision, bit 1 = its hard bit.  Sixteen steps
// at a time: g1, g2, g3 of all of them from shifted XORs of the decoded bits, the received values gathered with the running interleaver
// index into words that line up with them.  Returns errors | compared << 16.
template <int NG, class Half, class Rx>
LM_FN uint32_t reencode_errors(int n2, Half half, Rx rx) {
    constexpr int VALS = NG == 2 ? 3 : 6, PERIOD = NG == 2 ? 22 : 6;
    int pos = kInterleaveA, left = PERIOD;
    uint32_t prev = 0, errors = 0, compared = 0;
    for (int h = 0; 16 * h < n2; ++h) {
        const uint32_t D = ((uint32_t)half(h) << 4) | prev;                 // d[t] at bit t - 16h + 4, zeros before the block
        prev = D >> 16;
        const uint32_t g[3] = { (D >> 4) ^ (D >> 3) ^ D, (D >> 4) ^ (D >> 2) ^ (D >> 1) ^ D, (D >> 4) ^ (D >> 3) ^ (D >> 2) ^ D };      // bit b: step 16h + b
        uint32_t r[3] = { 0, 0, 0 }, v[3] = { 0, 0, 0 };
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (16 * h + 2 * u < n2) {
                const bool is_short = --left == 0;
                left = is_short ? PERIOD : left;
#pragma unroll
                for (int k = 0; k < VALS; ++k) {
                    if (k < VALS - 1 || !is_short) {
                        const int gen = NG == 2 ? (k == 1 ? 1 : 0) : k % 3, step = 2 * u + (NG == 2 ? (k == 2 ? 1 : 0) : k / 3);
                        const uint32_t x = rx(interleave_next(pos, kInterleaveA, kType345));
                        v[gen] |= (x & 1u) << step;
                        r[gen] |= (x >> 1) << step;
                    }
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NG; ++q) {
            errors += (uint32_t)__builtin_popcount((r[q] ^ g[q]) & v[q]);
            compared += (uint32_t)__builtin_popcount(v[q]);
        }
    }
    return errors | (compared << 16);
}

// A lane's steps 2-3 behind its front end: cls as forward's; io.dec_st / io.dec_ld its decision words, io.out_st / io.out_ld its column
// of the decoded halves.  count: also the channel bit errors (else 0).
template <int NG, bool BITS, class Cls, class Io>
LM_FN uint32_t decode_kind(int n2, bool count, Cls cls, Io& io) {
    forward<NG, BITS ? kSrcBits : kSrcClasses>(n2, cls, [&](int u, uint32_t w) { io.dec_st(u, w); });
    traceback(n2, [&](int u) { return io.dec_ld(u); }, [&](int h, uint32_t half) { io.out_st(h, half); });
    if (!count) return 0u;
    return reencode_errors<NG>(n2, [&](int h) { return io.out_ld(h); }, [&](int p) -> uint32_t {
        return BITS ? 1u | (bfe_u(cls(p >> 5), 31u - (uint32_t)(p & 31), 1u) << 1) : bfe_u(cls(p >> 4), 2u * (uint32_t)(p & 15), 2u);
    });
}
// ... of either coded kind (ng is workgroup-uniform)
template <bool BITS, class Cls, class Io>
LM_FN uint32_t decode_lane(int ng, int n2, bool count, Cls cls, Io& io) {
    return ng == 2 ? decode_kind<2, BITS>(n2, count, cls, io) : decode_kind<3, BITS>(n2, count, cls, io);
}

// The workgroup's decoded rows -> memory, the lane's share: write_rows of lmac_core.hpp for the whole 8-bit units of a row, then the four
// bits behind them (type2 = 8 k + 4 for both coded kinds), a row per lane.
template <class Half, class St8, class St4>
LM_FN void write_rows(int lane, int rows_here, int type2, bool wide, Half half, St8 st8, St4 st4) {
    tetra_lmac::write_rows(lane, rows_here, type2 & ~7, wide, half, st8, st4);
    if ((type2 & 4) && lane < rows_here) {
        const int d = (type2 >> 2) - 1;
        st4(lane, d, spread4(((uint32_t)half(d >> 2, lane) >> (4 * (d & 3))) & 0xfu));
    }
}

// TCH/7.2 is descrambling alone.  The workgroup's share of its rows, a dword = four bits at a time: seq(w, q) = word w of what row q's
// bytes are XORed with as bits (byte rows: the scrambling sequence; frames: the descrambled block, the "bytes" then zero), ld4(q, d) /
// st4(q, d, v) = bytes 4d .. 4d+3 of row q.  Every byte is masked to its low bit.
template <class Seq, class Ld4, class St4>
LM_FN void passthrough_rows(int lane, int rows_here, Seq seq, Ld4 ld4, St4 st4) {
    constexpr int kDwords = kType345 / 4;
    for (int i = lane; i < rows_here * kDwords; i += kLanes) {
        const int q = i / kDwords, d = i - q * kDwords;
        st4(q, d, (ld4(q, d) ^ bbk_bytes(seq(d >> 3, q), d & 7)) & 0x01010101u);
    }
}

}  // namespace tetra_tch
