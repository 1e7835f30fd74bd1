// list_core.hpp -- lane-level code of the CRC-aided list decoding of CRC-failed blocks (include/ext/tetra_list.h): margin collection,
// candidate selection, candidate traceback with the backward CRC.  Compiled by hipcc into the rescue kernel (k_list_rescue in
// tetra_lmac.hip) and by g++ (-DTETRA_HOST_EMUL) into tests/emul/lmac_list_emul.cpp, like lmac_core.hpp.
//
// A lane holds one block whose maximum-likelihood (ML) path -- the traceback from state 0 after the flush steps, ties to the even
// predecessor: what decode_hard / decode_soft wrote -- failed the CRC.  The block has N = type2 + kFlush trellis steps; s_t is the ML
// path's state after step t.
//   margin        D_t = the difference acs_step forms into state s_t at step t (even predecessor minus odd), Delta_t = |D_t|
//   candidate(t)  the traceback from state 0 with the single decision at (step t, state s_t) inverted: the best path that merges into
//                 the ML path at step t
//   order         ascending Delta_t, ties by ascending t, all N steps
//   rescue        the first of the first T candidates whose CRC is good wins; rank = its 1-based place in the order
// The lane runs (1) the ML traceback again from the launch's decision scratch -- its decoded halves give s_t: the encoder register holds
// the four newest input bits, newest at bit 3 --, (2) the forward recursion once more on its staged block with a probe that picks D_t out
// of the step's eight difference registers and keeps the T smallest keys Delta_t << 16 | t in a sorted list of registers, (3) up to T
// tracebacks, each with one decision inverted (viterbi_traceback's flip hook).  No decision word is written: the scratch keeps the
// decoder's.
//
// Range of the key.  Hard routes: metrics in units of 127 stay inside [-584, 604] (lmac_core.hpp), |D| <= 1188 + 4.  Soft route: raw
// 6-bit values, |D| <= 2540 + 864 Q + 4 Q = 29448 (soft_core.hpp) -- inside int16, whose SIGN the decision already relies on, and
// below 2^15, so Delta << 16 | t (t < 292 < 2^16) is a positive 32-bit number and unsigned order on keys is the order above.
#pragma once

#include "lmac_core.hpp"
#include "soft_core.hpp"

namespace tetra_list {

using namespace tetra_lmac;

constexpr int kMaxCandidates = 8;
constexpr int kDefaultCandidates = 4;
constexpr uint32_t kNoKey = 0xffffffffu;

// s_t for 0 <= t < n2 + kFlush from the ML path's decoded halves (half(h) = bits 16h .. 16h+15, bit 16h + b at bit b; zeros before
// the block and in the flush steps)
template <class Half>
LM_FN uint32_t ml_state(int t, int n2, Half half) {
    const int h = t >> 4;
    const uint32_t cur = h < n2 / 16 ? (uint32_t)half(h) & 0xffffu : 0u, prev = h > 0 ? (uint32_t)half(h - 1) & 0xffffu : 0u;
    return (((cur << 16) | prev) >> ((t & 15) + 13)) & 15u;
}

// Delta of a step: D[i] = (difference into state i, into state i + 8)
// (a tree of seven bit selects on the three low bits of s: written as "register s & 7 of D", or as a chain of conditional moves, the
// compiler puts the eight registers into scratch memory and indexes them there)
LM_FN uint32_t margin(const Pk D[8], uint32_t s) {
    const uint32_t m0 = 0u - (s & 1u), m1 = 0u - ((s >> 1) & 1u), m2 = 0u - ((s >> 2) & 1u);
    const uint32_t a = select_bits(pk_bits(D[1]), pk_bits(D[0]), m0), b = select_bits(pk_bits(D[3]), pk_bits(D[2]), m0);
    const uint32_t c = select_bits(pk_bits(D[5]), pk_bits(D[4]), m0), e = select_bits(pk_bits(D[7]), pk_bits(D[6]), m0);
    const uint32_t bits = select_bits(select_bits(e, c, m1), select_bits(b, a, m1), m2);
    const int d = (int)(int16_t)(uint16_t)((s & 8u) ? bits >> 16 : bits & 0xffffu);
    return (uint32_t)(d < 0 ? -d : d);
}

// the kMaxCandidates smallest keys seen, ascending (a key is unique: it holds its step)
struct Best { uint32_t key[kMaxCandidates]; };
LM_FN void best_clear(Best& b) {
#pragma unroll
    for (int k = 0; k < kMaxCandidates; ++k) b.key[k] = kNoKey;
}
LM_FN void best_insert(Best& b, uint32_t key) {
#pragma unroll
    for (int k = 0; k < kMaxCandidates; ++k) {
        const uint32_t lo = key < b.key[k] ? key : b.key[k];
        key = key < b.key[k] ? b.key[k] : key;
        b.key[k] = lo;
    }
}
// the head of the list; the rest moves up
LM_FN uint32_t best_pop(Best& b) {
    const uint32_t head = b.key[0];
#pragma unroll
    for (int k = 0; k + 1 < kMaxCandidates; ++k) b.key[k] = b.key[k + 1];
    b.key[kMaxCandidates - 1] = kNoKey;
    return head;
}

// viterbi_forward's probe: half as ml_state's
template <class Half>
struct MarginProbe {
    int n2;
    Half half;
    Best& best;
    LM_MEM void operator()(int u, const Pk* De, const Pk* Do) const {
        best_insert(best, (margin(De, ml_state(2 * u, n2, half)) << 16) | (uint32_t)(2 * u));
        best_insert(best, (margin(Do, ml_state(2 * u + 1, n2, half)) << 16) | (uint32_t)(2 * u + 1));
    }
};
template <class Half>
LM_FN MarginProbe<Half> margin_probe(int n2, Half half, Best& best) { return MarginProbe<Half>{ n2, half, best }; }

// viterbi_traceback's flip: the decision met at step t
struct FlipAt {
    int t;
    LM_MEM uint32_t operator()(int step) const { return step == t ? 0xffffffffu : 0u; }
};

// (3): io as decode_hard's (dec_ld: the decoder's decision words; out_st receives every tried candidate's halves, so after a win they are
// the winner's -- and after none, the last loser's: the caller writes nothing then).  Returns the winner's rank, -1 if none of the first
// T passes.
template <class Io>
LM_FN int try_candidates(int type2, int T, Best best, Io& io) {
    int rank = -1;
    for (int k = 1; k <= T && rank < 0; ++k) {
        const uint32_t key = best_pop(best);
        if (traceback(type2, io, FlipAt{ (int)(key & 0xffffu) })) rank = k;
    }
    return rank;
}

// (1) - (3) for a lane on the hard routes (cls, BITS: as decode_hard's) ...
template <bool BITS, class Cls, class Io, class Half>
LM_FN int rescue_hard(int type345, int type2, int a, int T, Cls cls, Io& io, Half half) {
    (void)traceback(type2, io);
    Best best;
    best_clear(best);
    forward_hard<BITS>(type345, type2, a, cls, [](int, uint32_t) {}, margin_probe(type2, half, best));
    return try_candidates(type2, T, best, io);
}
// ... and on soft values (ld: as decode_soft's)
template <class Ld, class Io, class Half>
LM_FN int rescue_soft(int type345, int type2, int a, int T, Ld ld, Io& io, Half half) {
    (void)traceback(type2, io);
    Best best;
    best_clear(best);
    tetra_soft::forward(type345, type2, a, ld, [](int, uint32_t) {}, margin_probe(type2, half, best));
    return try_candidates(type2, T, best, io);
}

}  // namespace tetra_list
