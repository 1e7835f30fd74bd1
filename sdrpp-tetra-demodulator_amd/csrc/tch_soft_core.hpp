// tch_soft_core.hpp -- lane-level code of the coded circuit-mode data channels TCH/4.8 and TCH/2.4 decoded from SOFT values
// (include/ext/tetra_tch_soft.h).  Compiled by hipcc into k_tch_rows_soft / k_tch_frames_soft (tetra_lmac.hip) and by g++
// (-DTETRA_HOST_EMUL) into tests/emul/lmac_tch_soft_emul.cpp, which holds it bit for bit against the reference's conv_cch_decode behind
// its own TCH puncturers.  It is the two headers beside it joined, and restates nothing they hold:
//   * front end       soft_core.hpp: a block is 432 biased bytes (soft value + 128) in type-4 order, four per word, descrambled by sign.
//                     From a ring: tetra_soft::soft_block with the SCH/F layout (both blocks of a NORM_1 burst; a frame of another burst
//                     type is 432 erasures).  From an int8 byte row: stage_row below, the row's words through bias_and_flip.
//   * forward         tch_core.hpp's forward<NG, kSrcSoft>: its schedule (the countdown to the short pair, 3 or 6 values a step pair),
//                     step_metrics / acs_step / decision_word; a value is the staged byte - 128, an absent one is masked to 0 (the
//                     reference depunctures onto zeros), the start metric is soft_core.hpp's kStartMetric = 2540 raw units.
//   * traceback       tetra_tch::traceback as it is (from state 0 behind the four flush steps, no CRC).
//   * bit errors      tetra_tch::reencode_errors<NG>; a position is compared where its staged byte is not 128 (a soft value of zero
//                     carries no decision) and its hard bit is 1 where the byte is below 128: bit_errors_soft's reading.
// TCH/7.2 is not coded and has no soft route.
//
// The int16 bound.  The packed path metrics (lmac_core.hpp: 16 states in 8 registers of two int16) are never renormalised, so every
// sum an add-compare-select forms has to stay inside int16 for |value| <= Q = 31 (soft_core.hpp's kQ; unchecked, as there).  A step's
// branch metric is +-(the step's values summed with signs), so |m| <= NG Q, and a step pair moves a path metric by at most the
// magnitudes of its values: VALS Q.  The flush steps add nothing.  With s0 = 2540 on state 0 and 0 elsewhere, after all pairs every
// metric lies inside [-T, s0 + T], T = pairs x VALS x Q, and an add-compare-select forms e = S[2i] + m, o = S[2i+1] - m (each inside
// [-T - NG Q, s0 + T + NG Q]) and their difference, |e - o| <= s0 + 2 T + 2 NG Q:
//     TCH/2.4   74 pairs of at most 6 Q = 186:  T = 13764;  sums within [-13857, 16397];  |e - o| <= 2540 + 27528 + 186 = 30254 < 32767
//     TCH/4.8  146 pairs of at most 3 Q =  93:  T = 13578;  sums within [-13640, 16180];  |e - o| <= 2540 + 27156 + 124 = 29820 < 32767
// (the short pairs carry one value fewer, which only lowers T: 13392 and 13392).  step_metrics' partial sums are at most 3 Q = 93.
// The reference keeps int16 sums as well and renormalises them to a minimum of 0 every 59 steps (osmo_conv.c:137-153, :642): its sums
// are those above less what it has subtracted so far, so it does not overflow on these values either; a renormalisation subtracts the
// same amount from every state and changes no comparison, and both make the same decisions.
#pragma once

#include "soft_core.hpp"
#include "tch_core.hpp"

namespace tetra_tch_soft {

using namespace tetra_tch;

constexpr int kSoftWords = tetra_soft::kSoftWords;        // 108 words = 432 staged bytes per lane
static_assert(kType345 == 4 * kSoftWords, "a TCH block fills the soft staging of SCH/F");

// The byte-row front end: the lane's row of 432 int8 soft values in type-5 order -> the staged block.  ld4(g) = values 4g .. 4g+3 of the
// row (first value in the low byte), rows: as lane_sequence's, st(g, word): as stage_block's.
template <class Rows, class Ld4, class St>
LM_FN void stage_row(uint32_t code, Rows rows, Ld4 ld4, St st) {
    uint32_t seq[kSeqWords] = {};
    lane_sequence(kType345, code, rows, [&](int w, uint32_t word) { seq[w] = word; });
#pragma unroll
    for (int g = 0; g < kSoftWords; ++g)
        st(g, tetra_soft::bias_and_flip(ld4(g), tetra_soft::nibble_mask((seq[g >> 3] >> (28 - 4 * (g & 7))) & 0xfu)));
}

// The frame front end: tetra_soft::soft_block for a job that carries no layout of its own -- a TCH block lies where SCH/F lies.
// bitnum(), frame_type(), rows, ring, ring_words, st: as soft_block's.
template <class Bitnum, class FrameType, class Rows, class Ring, class St>
LM_FN void frame_block(uint32_t code, Bitnum bitnum, FrameType frame_type, Rows rows, Ring ring, uint32_t ring_words, St st) {
    const BlockKind kind{ kLayoutSchF, kType345 };
    tetra_soft::soft_block(&kind, code, bitnum, frame_type, rows, ring, ring_words, st);
}

// A lane's steps 2-3 behind its front end: ld(w) = the lane's staged word w; io as tetra_tch::decode_kind's.  count: also the channel
// bit errors (else 0).
template <int NG, class Ld, class Io>
LM_FN uint32_t decode_kind(int n2, bool count, Ld ld, Io& io) {
    forward<NG, kSrcSoft>(n2, ld, [&](int u, uint32_t w) { io.dec_st(u, w); }, tetra_soft::kStartMetric);
    traceback(n2, [&](int u) { return io.dec_ld(u); }, [&](int h, uint32_t half) { io.out_st(h, half); });
    if (!count) return 0u;
    return reencode_errors<NG>(n2, [&](int h) { return io.out_ld(h); }, [&](int p) -> uint32_t {
        const uint32_t y = bfe_u(ld(p >> 2), 8u * (uint32_t)(p & 3), 8);      // soft value + 128
        return (y != 128u ? 1u : 0u) | (y < 128u ? 2u : 0u);
    });
}
// ... of either coded kind (ng is workgroup-uniform)
template <class Ld, class Io>
LM_FN uint32_t decode_lane(int ng, int n2, bool count, Ld ld, Io& io) {
    return ng == 2 ? decode_kind<2>(n2, count, ld, io) : decode_kind<3>(n2, count, ld, io);
}

}  // namespace tetra_tch_soft
