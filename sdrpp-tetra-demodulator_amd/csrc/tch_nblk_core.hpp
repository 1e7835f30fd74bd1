// tch_nblk_core.hpp -- the front end of TCH/4.8 and TCH/2.4 interleaved over N = 1, 4 or 8 blocks (include/ext/tetra_tch_nblk.h).
// Compiled by hipcc into k_tch_nblk / k_tch_nblk_soft (tetra_lmac.hip) and by g++ (-DTETRA_HOST_EMUL) into
// tests/emul/lmac_tch_nblk_emul.cpp.  A lane builds its block out of the N received rows its window names and hands it to
// tetra_tch::decode_lane / tetra_tch_soft::decode_lane as they are: nothing behind the front end is restated here.
//
// The gather.  Output block b with window w[0..N), P = 432 / N; for p = 0 .. 431 with j = p mod N, i = p div N:
//     type3[p] = the descrambled value of received row w[j] at type-4 position t = 103 (j P + i + 1) mod 432
// and the decoders read an N = 1 block in type-4 order through the (432, 103) interleaver, so the lane stages
//     virtual type-4 position q = 103 (p + 1) mod 432  <-  type3[p].
// Walked a diagonal at a time (j outer, i inner): t advances by 103 and q by 103 N, both mod 432, from t = 103 (j P + 1) and
// q = 103 (j + 1); no division in the loop.  The scrambling sequence belongs to the RECEIVED row, so each diagonal fetches its row's
// sequence once (lane_sequence) and picks bit t of it.  A window entry outside [0, n_rows) is a lost burst: its P positions keep what the
// staging was cleared to (an erasure), and nothing is read for it.  For N = 1, q = t: the N = 1 block of tetra_tch.h / tetra_tch_soft.h.
#pragma once

#include "tch_soft_core.hpp"

namespace tetra_tch_nblk {

using namespace tetra_tch_soft;

constexpr bool valid_n(int n) { return n == 1 || n == 4 || n == 8; }

// Every position of the lane's block whose burst is there: take(r, t, q, bit) = received row r, its type-4 position t and the bit of its
// scrambling sequence there, to be staged at virtual position q.  win(j): the window's entry j; code(r): the scrambling code of received
// row r; rows: as lane_sequence's; seq_st(w, word) / seq_ld(w): a place for one sequence (kSeqWords words) that the lane owns.
// Returns the number of lost bursts of the window.
// (Fetching a diagonal's positions 27 at a time before staging any, with the next diagonal's window entry and code requested a diagonal
// ahead, was built and measured: 152 VGPRs for times a little above and a little below this loop's, so the gather waits less for its
// loads' latency than for their issue -- every one touches 64 cache lines -- and the plain loop stayed.  DESIGN.md 8.3.)
template <class Win, class Code, class Rows, class SeqSt, class SeqLd, class Take>
LM_FN int gather(int n, int n_rows, Win win, Code code, Rows rows, SeqSt seq_st, SeqLd seq_ld, Take take) {
    const int P = kType345 / (n > 0 ? n : 1), dq = (kInterleaveA * n) % kType345;
    int lost = 0;
    for (int j = 0; j < n; ++j) {
        const int r = win(j);
        if ((uint32_t)r >= (uint32_t)n_rows) {
            ++lost;
            continue;
        }
        lane_sequence(kType345, code(r), rows, seq_st);
        int t = (kInterleaveA * (j * P + 1)) % kType345, q = (kInterleaveA * (j + 1)) % kType345;
#pragma unroll 4
        for (int i = 0; i < P; ++i) {
            take(r, t, q, bfe_u(seq_ld(t >> 5), 31u - (uint32_t)(t & 31), 1u));
            t += kInterleaveA;
            t -= t >= kType345 ? kType345 : 0;
            q += dq;
            q -= q >= kType345 ? kType345 : 0;
        }
    }
    return lost;
}

// Hard bits: the block as soft classes, 16 per word as descramble_chunk leaves them (kClsWords + 1 words, cleared by the caller: class 0
// is the erasure).  byte(r, t) = byte t of received row r; or_cls(w, bits): word w |= bits.  Returns non-zero unless every burst of the
// window is there and every byte met is 0 or 1 (then classes_to_bits may follow).
template <class Win, class Code, class Rows, class SeqSt, class SeqLd, class Byte, class OrCls>
LM_FN uint32_t gather_hard(int n, int n_rows, Win win, Code code, Rows rows, SeqSt seq_st, SeqLd seq_ld, Byte byte, OrCls or_cls) {
    uint32_t dirty = 0;
    const int lost = gather(n, n_rows, win, code, rows, seq_st, seq_ld, [&](int r, int t, int q, uint32_t bit) {
        const uint32_t v = byte(r, t);
        dirty |= v & 0xfeu;
        or_cls(q >> 4, soft_class(v ^ bit) << (2 * (q & 15)));
    });
    return dirty | (uint32_t)lost;
}

LM_FN uint32_t rev32(uint32_t x) {
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
    return __builtin_bitreverse32(x);
#else
    x = (x >> 16) | (x << 16);
    x = ((x & 0xff00ff00u) >> 8) | ((x & 0x00ff00ffu) << 8);
    x = ((x & 0xf0f0f0f0u) >> 4) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x & 0xccccccccu) >> 2) | ((x & 0x33333333u) << 2);
    return ((x & 0xaaaaaaaau) >> 1) | ((x & 0x55555555u) << 1);
#endif
}
// the upper bit of each of a word's sixteen classes (set for a strong 1), class u at bit u
LM_FN uint32_t class_signs(uint32_t x) {
    x = (x >> 1) & 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0f0f0f0fu;
    x = (x | (x >> 4)) & 0x00ff00ffu;
    return (x | (x >> 8)) & 0xffffu;
}
// A block without erasures, in place: classes (bit i at bits 2 (i & 15) .. of word i >> 4) -> packed bits (bit i at bit 31 - (i & 31) of
// word i >> 5), what decode_lane<true> reads.  Word k is written after words 2k and 2k + 1 were read, k <= 2k; word kClsWords is the
// cleared spare word.
template <class Ld, class St>
LM_FN void classes_to_bits(Ld ld, St st) {
#pragma unroll
    for (int k = 0; k < kSeqWords; ++k) st(k, rev32(class_signs(ld(2 * k)) | (class_signs(ld(2 * k + 1)) << 16)));
}

// Soft values: the block as the staged bytes of soft_core.hpp (value + 128, four per word; kSoftWords words, cleared by the caller to
// 0x80808080: a value of zero carries no decision).  value(r, t) = the int8 at position t of received row r as 0 .. 255; st8(q, y): byte q
// of the staging.  A value is negated where its row's sequence has a 1: bias_and_flip's bytes for |value| <= 31.
template <class Win, class Code, class Rows, class SeqSt, class SeqLd, class Value, class St8>
LM_FN void gather_soft(int n, int n_rows, Win win, Code code, Rows rows, SeqSt seq_st, SeqLd seq_ld, Value value, St8 st8) {
    (void)gather(n, n_rows, win, code, rows, seq_st, seq_ld, [&](int r, int t, int q, uint32_t bit) {
        const uint32_t x = value(r, t);
        st8(q, (bit ? 128u - x : 128u + x) & 0xffu);
    });
}

}  // namespace tetra_tch_nblk
