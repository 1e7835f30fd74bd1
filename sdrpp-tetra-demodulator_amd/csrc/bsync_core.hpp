// bsync_core.hpp -- the burst synchroniser's logic (include/tetra_burst_sync.h), shared by the gfx950 kernel
// (tetra_burst_sync.hip) and its host builds (tests/emul/bsync_emul.cpp, bsync_tol_emul.cpp through bsync_lane_io.hpp, -DTETRA_HOST_EMUL).
//
// Contract: for one channel, one call over n_new bits leaves exactly the state, and reports exactly the frames, that the
// reference's tetra_burst_sync_in() (src/decoder/src/phy/tetra_burst_sync.c:54-155) produces when it is handed the same
// bits ONE BIT PER CALL.  (The reference consumes at most one frame per call and its 4096-byte buffer drops the oldest
// bits when a call overfills it, :38-51, so its result depends on how the caller chunks the stream; one bit per call is
// the chunking-independent limit of the small stream buffers the plugin feeds it, src/dsp/osmotetra_dec.h:182-184.)
//
// The per-bit calls are not replayed one by one.  The stream of a call is laid out once in "coordinates": the carried
// buffer occupies [kOff - bits_in_buf, kOff), the new bits [kOff, kOff + n_new); bits are packed 32 per word, MSB first.
// Three match bitmaps (sync, normal 1, normal 2 training sequence truly present at x and inside the stream) are built
// in parallel.  The state machine then jumps from event to event:
//   UNLOCKED     the first call that can search is A1 = max(A + 1, Bx + 1020) (buffer [Bx, A), :66-71).  Every later call
//                re-scans the whole buffer, but the only position that was not already rejected by an earlier call is the
//                newest one that fits, so the hit is the first true sync match p >= Bx + 21 and it is found by the call
//                A = max(A1, p + 38).  The first 21 buffer positions are special: the reference's pre-filter is
//                misaligned there (tetra_burst.c:289-296), so a true match only counts if that filter fires too; if the
//                bitmap shows a true match in that zone the call is evaluated literally (literal_find) -- rare.
//   KNOW_FSTART  nothing happens until the call A = max(A + 1, next_frame_start) (:90-92); that call moves the buffer start
//                to the frame start and falls through into LOCKED (:93-104).
//   LOCKED       a frame is consumed by every call that finds >= 510 bits buffered (:105-150): search [Bx, A) for the first
//                of {sync, normal 1, normal 2}; sync at 214 / normal at 244 -> burst reported with its type; sync
//                elsewhere or nothing found -> UNLOCKED; normal elsewhere -> frame dropped, still LOCKED.
// All bit numbers are uint32 and wrap like the reference's unsigned ints.
//
// Tolerant lock (include/ext/tetra_sync_tol.h; opt-in, a departure from the reference): UNLOCKED and KNOW_FSTART as above, but a LOCKED
// call looks only at the expected positions of the frame -- sync at 214, normal 1 / 2 at 244 --, accepts up to tol_sync / tol_norm bit
// errors there (tolerant_frame_eval) and falls back to UNLOCKED only behind max_miss consecutive frames without a candidate
// (first_unlock).  Only the sync bitmap is needed then.
//
// Hand-over (include/ext/tetra_handover.h; opt-in, a departure from the reference): a fourth state, kAssist, in which the channel looks
// for a training sequence only around the frame start it inherited from a donor; its fields (Assist) live beside State.  A third policy,
// AssistLock, wraps the handle's rule and adds that state to walk(); RefLock and TolLock compile walk() without it.
//
// One walk over the events, walk(), serves both: the rule is a small policy object (RefLock, TolLock) that says what a LOCKED call
// reports and how a literal call in UNLOCKED is answered; run() and run_tolerant() bind walk() to their rule.  Steps 1 and 4 of the kernel -- packing the stream, expanding the listed
// frames, writing the carried buffer back -- are lane code here too (stage_thread, write_thread), so the host build runs the kernel's text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define BS_FN __device__ __forceinline__
#define BS_MFN __device__ __forceinline__
#else
#define BS_FN static inline
#define BS_MFN inline               // (member functions: `static` would mean something else)
#endif

namespace bsync_core {

constexpr int kOff = 4096;          // coordinate of the first new bit = sizeof(trs->bitbuf), tetra_burst_sync.h:15
constexpr int kBuf = 4096;
constexpr int kTs = 510;            // TETRA_BITS_PER_TS
constexpr int kLook = 64;           // zero bits kept past the end of the stream for window reads
enum { kUnlocked = 0, kKnowFstart = 1, kLocked = 2 };                   // enum rx_state, tetra_burst_sync.h:6-10
constexpr int kAssist = 3;          // ... and the hand-over's state beside them (include/ext/tetra_handover.h): not the reference's
enum { kNorm1 = 0, kNorm2 = 1, kNorm3 = 2, kSync = 3, kExt = 4 };       // enum tetra_train_seq, tetra_burst.h:26-32

struct State {                      // struct tetra_rx_state without its bitbuf (kept separately, one byte per bit)
    int32_t state;
    uint32_t bits_in_buf;
    uint32_t bitbuf_start_bitnum;
    uint32_t next_frame_start_bitnum;
};

// first 22 bits of y (sync), n, p, q (normal 1-3), x (extended) -- EN 300 392-2 9.4.4.3.2-4 -- MSB first, and the
// remaining 16 bits of y
constexpr uint32_t kHeadY = 0x30673a, kHeadN = 0x343a74, kHeadP = 0x1e90de, kHeadQ = 0x2dc1ad, kHeadX = 0x2743a7;
constexpr uint32_t kTailY = 0x7067;

constexpr int stream_words(int max_new) { return (kOff + max_new + kLook + 31) / 32 + 2; }

// ---- packed stream access -------------------------------------------------------------------------------------------
BS_FN uint32_t get_bit(const uint32_t* s, int x) { return (s[x >> 5] >> (31 - (x & 31))) & 1u; }
// bits x .. x+len-1 (len <= 32) as a number, first bit most significant
BS_FN uint32_t window(const uint32_t* s, int x, int len) {
    const uint64_t two = ((uint64_t)s[x >> 5] << 32) | s[(x >> 5) + 1];
    return (uint32_t)(two >> (64 - len - (x & 31))) & (uint32_t)((1ull << len) - 1);
}

// 32 stream bits starting k bits after the start of word w (k = 0..63), first bit most significant
BS_FN uint32_t shifted_word(uint32_t w0, uint32_t w1, uint32_t w2, int k) {
    const uint32_t hi = k < 32 ? w0 : w1, lo = k < 32 ? w1 : w2;
    const int r = k & 31;
    return r == 0 ? hi : (uint32_t)((((uint64_t)hi << 32) | lo) >> (32 - r));
}

BS_FN uint32_t bit_reverse(uint32_t v) {
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
    return __builtin_bitreverse32(v);
#else
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    return (v >> 16) | (v << 16);
#endif
}

// bit b (LSB = position 32w) set where positions lo <= 32w + b < hi
BS_FN uint32_t range_mask(int w, int lo, int hi) {
    int a = lo - 32 * w, b = hi - 32 * w;
    a = a < 0 ? 0 : a;
    b = b > 32 ? 32 : b;
    if (a >= b) return 0u;
    const uint32_t upto_b = b == 32 ? 0xffffffffu : ((1u << b) - 1u);
    return upto_b & (0xffffffffu << a);
}

// match bits of the 32 positions 32w .. 32w+31 (LSB = position 32w) for the three sequences; a position counts only if
// the whole sequence lies inside [x0, xe).  Bit-sliced: for every offset k into the sequence, the 32 candidate windows'
// k-th bits are one funnel-shifted word, AND-ed (or AND-NOT-ed) into the three running match words.
// NORMAL = false: the sync bitmap alone; m_n1 / m_n2 are left as they are.
template <bool NORMAL = true>
BS_FN void match_word(const uint32_t* s, int w, int x0, int xe, uint32_t& m_sync, uint32_t& m_n1, uint32_t& m_n2) {
    const uint32_t w0 = s[w], w1 = s[w + 1], w2 = s[w + 2];
    uint32_t ay = 0xffffffffu, an = 0xffffffffu, ap = 0xffffffffu;
    constexpr uint64_t seq_y = ((uint64_t)kHeadY << 16) | kTailY;          // 38 bits, first bit = bit 37
#pragma unroll
    for (int k = 0; k < 38; ++k) {
        const uint32_t v = shifted_word(w0, w1, w2, k);
        ay &= ((seq_y >> (37 - k)) & 1u) ? v : ~v;
        if (NORMAL && k < 22) {
            an &= ((kHeadN >> (21 - k)) & 1u) ? v : ~v;
            ap &= ((kHeadP >> (21 - k)) & 1u) ? v : ~v;
        }
    }
    // ay/an/ap: bit 31 - b = position 32w + b  ->  bit b
    m_sync = bit_reverse(ay) & range_mask(w, x0, xe - 38 + 1);
    if (NORMAL) {
        m_n1 = bit_reverse(an) & range_mask(w, x0, xe - 22 + 1);
        m_n2 = bit_reverse(ap) & range_mask(w, x0, xe - 22 + 1);
    }
}

// match_word's sync bitmap alone (the tolerant lock needs no other)
BS_FN uint32_t match_word_sync(const uint32_t* s, int w, int x0, int xe) {
    uint32_t m_sync = 0, none = 0;
    match_word<false>(s, w, x0, xe, m_sync, none, none);
    return m_sync;
}

// first set bit of bitmap m (bit x at word x>>5, bit x&31) in [a, b), or -1
BS_FN int first_set(const uint32_t* m, int a, int b) {
    if (a >= b) return -1;
    for (int w = a >> 5; w <= (b - 1) >> 5; ++w) {
        uint32_t v = m[w];
        if (w == (a >> 5)) v &= 0xffffffffu << (a & 31);
        if (w == ((b - 1) >> 5) && ((b & 31) != 0)) v &= (1u << (b & 31)) - 1u;
        if (v) return 32 * w + __builtin_ctz(v);
    }
    return -1;
}

// tetra_find_train_seq() (tetra_burst.c:271-341) evaluated literally on the packed stream, buffer = [bx, bx + n)
BS_FN int literal_find(const uint32_t* s, int bx, int n, uint32_t mask, int& offs) {
    uint32_t filter = 0;
    for (int i = 0; i < 20; ++i) filter = (filter << 1) | get_bit(s, bx + i);
    for (int cur = 0; cur < n; ++cur) {
        filter = ((filter << 1) | get_bit(s, bx + cur + 21)) & 0x3fffffu;
        if (filter != kHeadY && filter != kHeadN && filter != kHeadP && filter != kHeadQ && filter != kHeadX) continue;
        const int remain = n - cur, x = bx + cur;
        if ((mask & (1u << kSync)) && remain >= 38 && window(s, x, 22) == kHeadY && window(s, x + 22, 16) == kTailY) { offs = cur; return kSync; }
        if ((mask & (1u << kNorm1)) && remain >= 22 && window(s, x, 22) == kHeadN) { offs = cur; return kNorm1; }
        if ((mask & (1u << kNorm2)) && remain >= 22 && window(s, x, 22) == kHeadP) { offs = cur; return kNorm2; }
        // normal 3 / extended are never enabled by the synchroniser
    }
    return -1;
}

// `first(m, a, b)` below is the "first set bit of bitmap m in [a, b)" primitive: first_set on the host, a wave-cooperative
// version (one word per lane + ballot) in the kernel, where all 64 lanes run the state machine in lock step.

// the LOCKED state's search over the buffer [bx, bx + n), n >= 510: first of {sync, normal 1, normal 2}.
// m_any = m_sync | m_n1 | m_n2 answers the common case with one search.
template <class First>
BS_FN int locked_find(const uint32_t* s, const uint32_t* m_sync, const uint32_t* m_n1, const uint32_t* m_n2, const uint32_t* m_any,
                      int bx, int n, int& offs, First first) {
    const uint32_t mask = (1u << kNorm1) | (1u << kNorm2) | (1u << kSync);
    const int p = first(m_any, bx, bx + n - 22 + 1);
    if (p < 0) return -1;
    if (p < bx + 21) return literal_find(s, bx, n, mask, offs);            // misaligned-filter zone: evaluate literally
    const bool is_sync = (m_sync[p >> 5] >> (p & 31)) & 1u;
    if (!is_sync || p + 38 <= bx + n) {
        offs = p - bx;
        return is_sync ? kSync : (((m_n1[p >> 5] >> (p & 31)) & 1u) ? kNorm1 : kNorm2);
    }
    // a sync sequence that does not fit the buffer any more: the three sequences separately
    const int ps = first(m_sync, bx + 21, bx + n - 38 + 1);
    const int p1 = first(m_n1, bx + 21, bx + n - 22 + 1);
    const int p2 = first(m_n2, bx + 21, bx + n - 22 + 1);
    int best = -1, type = -1;
    if (ps >= 0) { best = ps; type = kSync; }
    if (p1 >= 0 && (best < 0 || p1 < best)) { best = p1; type = kNorm1; }
    if (p2 >= 0 && (best < 0 || p2 < best)) { best = p2; type = kNorm2; }
    if (best >= 0) offs = best - bx;
    return type;
}

// ---- tolerant lock --------------------------------------------------------------------------------------------------------------------
struct Tolerance {                  // tetra_bsync_tolerance_t
    int32_t tol_norm;               // 0..4 bit errors accepted in a normal training sequence at 244
    int32_t tol_sync;               // 0..6 in the sync training sequence at 214
    int32_t max_miss;               // 1..255 consecutive frames without a candidate before the receiver unlocks
};
constexpr int kTolNormMax = 4, kTolSyncMax = 6, kMaxMissMax = 255;
constexpr bool tolerance_valid(const Tolerance& t) {           // (constexpr: host and device)
    return t.tol_norm >= 0 && t.tol_norm <= kTolNormMax && t.tol_sync >= 0 && t.tol_sync <= kTolSyncMax && t.max_miss >= 1 && t.max_miss <= kMaxMissMax;
}

// One tolerant LOCKED call on the frame [bx, bx + 510): Hamming distances of the three windows to y / n / p, the candidate with the
// smallest distance (ties: sync, normal 1, normal 2), or -1.  Nothing else of the buffer is looked at.
BS_FN int tolerant_frame_eval(const uint32_t* s, int bx, const Tolerance& t) {
    const int ds = __builtin_popcount(window(s, bx + 214, 22) ^ kHeadY) + __builtin_popcount(window(s, bx + 236, 16) ^ kTailY);
    const int d1 = __builtin_popcount(window(s, bx + 244, 22) ^ kHeadN);
    const int d2 = __builtin_popcount(window(s, bx + 244, 22) ^ kHeadP);
    int type = -1, best = 0;
    if (ds <= t.tol_sync) { type = kSync; best = ds; }
    if (d1 <= t.tol_norm && (type < 0 || d1 < best)) { type = kNorm1; best = d1; }
    if (d2 <= t.tol_norm && (type < 0 || d2 < best)) { type = kNorm2; best = d2; }
    return type;
}

// The consecutive-miss rule over n <= 64 frames evaluated side by side: bit k of pass_mask = frame k was reported.  The miss counter
// enters with misses_in (< max_miss).  index: the first frame at which the counter reaches max_miss (the receiver unlocks behind it and
// the frames after it are not LOCKED calls), or -1; misses: the counter behind frame `index` (0) or, without one, behind frame n - 1.
struct Unlock { int index; int misses; };
// the definition, frame by frame
BS_FN Unlock first_unlock(uint64_t pass_mask, int n, int misses_in, int max_miss) {
    int m = misses_in;
    for (int k = 0; k < n; ++k) {
        m = ((pass_mask >> k) & 1u) ? 0 : m + 1;
        if (m >= max_miss) return Unlock{ k, 0 };
    }
    return Unlock{ -1, m };
}
// the same with bit operations (the kernel's: pass_mask is a ballot).  A run that reaches max_miss either started in the carried counter
// -- then frames 0 .. max_miss - misses_in - 1 all miss -- or lies inside the mask: max_miss consecutive miss bits, found by and-ing the
// mask with shifted copies of itself, doubling the covered length.  The first kind ends no later than any of the second.
BS_FN Unlock first_unlock_bits(uint64_t pass_mask, int n, int misses_in, int max_miss) {
    if (n <= 0) return Unlock{ -1, misses_in };
    const uint64_t all = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    const uint64_t pass = pass_mask & all, miss = ~pass_mask & all;
    const int need = max_miss - misses_in;                      // frames still to miss for the carried run (>= 1)
    if (need <= n) {
        const uint64_t head = need >= 64 ? ~0ull : ((1ull << need) - 1ull);
        if ((miss & head) == head) return Unlock{ need - 1, 0 };
    }
    if (max_miss <= n) {
        uint64_t x = miss;                                      // bit j: frames j .. j + have - 1 all miss
        for (int have = 1; have < max_miss;) {
            const int sh = have < max_miss - have ? have : max_miss - have;
            x &= x >> sh;
            have += sh;
        }
        if (x) return Unlock{ __builtin_ctzll(x) + max_miss - 1, 0 };
    }
    if (!pass) return Unlock{ -1, misses_in + n };
    return Unlock{ -1, n - 1 - (63 - __builtin_clzll(pass)) };  // the misses behind the last reported frame
}

// ---- the two lock rules -----------------------------------------------------------------------------------------------------------------
// What a rule says to walk():
//   locked(s, bx, n, first)   one LOCKED call on the buffer [bx, bx + n), n >= 510: what tetra_burst_sync_in reports for its first frame
//                             (the rx_cb type, or -1) and whether the receiver falls back to UNLOCKED behind it;
//   literal(s, bx1, a1, xe, offs, a)   UNLOCKED with a true sync match in the misaligned-filter zone of the buffer that starts at bx1, first
//                             call a1: the literal search's result and offset, and in `a` the call that has been evaluated.
struct FrameEval { int reported; bool unlocks; };

// The reference's rule (tetra_burst_sync.c:105-150) on the three bitmaps and their union.  On a buffer of exactly one frame it is a
// pure function of the bitmaps: frames in LOCKED steady state can be evaluated side by side, one per lane (walk()'s `batch`).
struct RefLock {
    static constexpr bool kAssists = false;
    const uint32_t *m_sync, *m_n1, *m_n2, *m_any;
    template <class First> BS_MFN FrameEval locked(const uint32_t* s, int bx, int n, First first) const {
        int offs = 0;
        const int rc = locked_find(s, m_sync, m_n1, m_n2, m_any, bx, n, offs, first);
        FrameEval e = { -1, false };
        if (rc == kSync) {
            if (offs == 214) e.reported = rc;
            else e.unlocks = true;
        } else if (rc == kNorm1 || rc == kNorm2) {
            if (offs == 244) e.reported = rc;
        } else {
            e.unlocks = true;
        }
        return e;
    }
    BS_MFN int literal(const uint32_t* s, int bx1, int a1, int, int& offs, int& a) const {      // call by call
        a = a1;
        return literal_find(s, bx1, a1 - bx1, 1u << kSync, offs);
    }
};
BS_FN FrameEval locked_frame_eval(const uint32_t* s, const uint32_t* m_sync, const uint32_t* m_n1, const uint32_t* m_n2, const uint32_t* m_any,
                                  int bx) {
    return RefLock{ m_sync, m_n1, m_n2, m_any }.locked(s, bx, kTs, [](const uint32_t* m, int a, int b) { return first_set(m, a, b); });
}

// The tolerant rule: tolerant_frame_eval on the first 510 bits of the buffer and the channel's miss counter `misses`, carried from call
// to call.  A batch() evaluates its frames with tolerant_frame_eval, applies first_unlock to them with the same counter and leaves it
// as locked() does.  Only the sync bitmap is read.
struct TolLock {
    static constexpr bool kAssists = false;
    Tolerance tol;
    int& misses;
    template <class First> BS_MFN FrameEval locked(const uint32_t* s, int bx, int, First) {
        FrameEval e = { tolerant_frame_eval(s, bx, tol), false };
        misses = e.reported >= 0 ? 0 : misses + 1;
        if (misses >= tol.max_miss) { e.unlocks = true; misses = 0; }
        return e;
    }
    // Until the buffer is full its start stays bx1, and the calls a1, a1 + 1, ... search the same positions plus one more each: what an
    // earlier call rejected stays rejected, so the first call that finds anything finds the first position p that passes anywhere in
    // [bx1, lim), and it is the call a = max(a1, p + 38).  One literal search over the whole stretch stands for all of them, with the
    // same result.  (The reference's rule evaluates such a buffer call by call -- up to 3076 literal searches of up to 4096 positions
    // each on one wavefront, where this is one.  A flywheel that unlocks 16 frames late lands on such a buffer whenever the timing has
    // jumped by about 300 bits.)
    BS_MFN int literal(const uint32_t* s, int bx1, int a1, int xe, int& offs, int& a) const {
        const int lim = xe < bx1 + kBuf ? xe : bx1 + kBuf;
        const int rc = literal_find(s, bx1, lim - bx1, 1u << kSync, offs);
        if (rc >= 0) a = (bx1 + offs + 38 > a1) ? bx1 + offs + 38 : a1;
        else a = lim > a1 ? lim : a1;
        return rc;
    }
};

// ---- hand-over (include/ext/tetra_handover.h; opt-in, a departure from the reference) ------------------------------------------------------
// A channel that inherited its frame timing from a donor is in the state kAssist: it knows where its next frame should start (`expect`, an
// absolute bit number) and looks for a training sequence only there, `window` bits either side, once per slot period, for at most
// `slots_left` periods.  The fields live beside State, one Assist per channel; its first three words are tetra_handover_status_t.
enum { kHoNone = 0, kHoPending = 1, kHoLocked = 2, kHoExpired = 3, kHoRefused = 4 };       // TETRA_HANDOVER_*
struct Assist {
    int32_t status;                 // kHo*
    int32_t waited;                 // slot periods ASSIST has advanced
    int32_t offset;                 // found frame start - expected frame start, in bits (once locked)
    uint32_t expect;                // absolute bit number of the expected frame start
    int32_t window;                 // W: 0..127
    int32_t slots_left;
    int32_t result;                 // for the apply kernel, which clears it: 1 + waited on the lock, -1 on expiry, 0 nothing
    int32_t reserved;
};
constexpr int kAssistWords = (int)(sizeof(Assist) / 4);
constexpr int kWindowMax = 127, kAssistSlotsMax = 255;

// a frame that starts at x carries the sync sequence exactly at 214, or normal sequence 1 or 2 exactly at 244
BS_FN bool assist_match(const uint32_t* s, int x) {
    const uint32_t n = window(s, x + 244, 22);
    return n == kHeadN || n == kHeadP || (window(s, x + 214, 22) == kHeadY && window(s, x + 236, 16) == kTailY);
}
// The candidates ex + d in the order d = 0, +1, -1, ..., +w, -w, none in front of the buffer's start bx: the first that matches, or -1.
// All of [ex - w, ex + w + 510) lies in the stream.
BS_FN int assist_find(const uint32_t* s, int bx, int ex, int w) {
    for (int i = 0; i <= 2 * w; ++i) {
        const int d = (i & 1) ? (i + 1) / 2 : -(i / 2);
        if (ex + d >= bx && assist_match(s, ex + d)) return ex + d;
    }
    return -1;
}
// The third policy of walk(): the handle's own lock rule (RefLock, TolLock) for everything LOCKED and UNLOCKED, and the channel's Assist
// for the state kAssist.
template <class Inner> struct AssistLock {
    static constexpr bool kAssists = true;
    Inner& inner;
    Assist& as;
    template <class First> BS_MFN FrameEval locked(const uint32_t* s, int bx, int n, First first) { return inner.locked(s, bx, n, first); }
    BS_MFN int literal(const uint32_t* s, int bx1, int a1, int xe, int& offs, int& a) const { return inner.literal(s, bx1, a1, xe, offs, a); }
};

// Runs the state machine over the new bits under the rule `lock`.  emit(f, bx, type, bitnum) is called for the f-th consumed frame
// (buffer coordinate of its first bit, the reference's rx_cb type or -1, absolute bit number of its first bit).  On return
// st holds the new state and carry_x the coordinate of the first bit that stays buffered ([carry_x, xe) = the new bitbuf).
// batch(bx, K, f0, abs_bx, unlocked): LOCKED steady state (the fed position a equals the buffer start bx, so every call consumes
// exactly the next 510 bits): evaluate up to K whole frames [bx + 510 k, bx + 510 (k + 1)) and emit them as frames f0, f0 + 1, ... up to
// and including the first one that unlocks the receiver; returns how many it consumed (0 = not taken: the serial path runs).  The
// kernel does this one frame per lane -- ~70 dependent event steps per second of signal become two -- the host emulation in a loop.
template <class Lock, class First, class Emit, class Batch>
BS_FN int walk(State& st, const uint32_t* s, const uint32_t* m_sync, int n_new, int& carry_x, First first, Emit emit, Batch batch, Lock& lock) {
    const int x0 = kOff - (int)st.bits_in_buf, xe = kOff + n_new;
    const uint32_t abs0 = st.bitbuf_start_bitnum;               // absolute bit number of coordinate x0
    auto abs_of = [&](int x) { return abs0 + (uint32_t)(x - x0); };
    int state = st.state, bx = x0, a = kOff, frames = 0;
    uint32_t nfs = st.next_frame_start_bitnum;

    auto locked_call = [&]() {                                  // buffer [bx, a)
        const int n = a - bx;
        if (n < kTs) return;
        const FrameEval e = lock.locked(s, bx, n, first);
        if (e.unlocks) state = kUnlocked;
        emit(frames++, bx, e.reported, abs_of(bx));
        bx += kTs;
        nfs += kTs;
    };

    while (a < xe) {
        if constexpr (Lock::kAssists) {
            // kAssist: nothing happens until the call that has fed expect + W + 510 bits; that call tries the window.  A match moves the
            // buffer's start to the frame's and is LOCKED at once, the matched frame consumed in the same call like KNOW_FSTART's; a miss
            // moves on by one slot period and drops what lies in front of the next window; the last miss is UNLOCKED on what is buffered.
            if (state == kAssist) {
                Assist& as = lock.as;
                const int ex = x0 + (int)(int32_t)(as.expect - abs0);
                const int at = ex + as.window + kTs;
                if (at > xe) { a = xe; break; }
                a = at > a ? at : a;
                const int sx = assist_find(s, bx, ex, as.window);
                if (sx >= 0) {
                    bx = sx;
                    nfs = abs_of(bx) + (uint32_t)kTs;
                    state = kLocked;
                    as.status = kHoLocked;
                    as.offset = sx - ex;
                    as.result = 1 + as.waited;
                    locked_call();
                } else {
                    as.expect += (uint32_t)kTs;
                    as.waited += 1;
                    as.slots_left -= 1;
                    bx = (ex + kTs - as.window > bx) ? ex + kTs - as.window : bx;
                    if (as.slots_left <= 0) {
                        state = kUnlocked;
                        as.status = kHoExpired;
                        as.result = -1;
                    }
                }
                continue;
            }
        }
        if (state == kUnlocked) {
            const int a1 = (a + 1 > bx + 2 * kTs) ? a + 1 : bx + 2 * kTs;
            if (a1 > xe) { a = xe; break; }
            const int bx1 = (a1 - kBuf > bx) ? a1 - kBuf : bx;
            if (first(m_sync, bx1, bx1 + 21) >= 0) {        // a true match in the misaligned-filter zone: literal, as the rule has it
                int offs = 0;
                const int rc = lock.literal(s, bx1, a1, xe, offs, a);
                bx = bx1;
                if (rc >= 0) { nfs = abs_of(bx) + (uint32_t)offs + 296u; state = kKnowFstart; }
                continue;
            }
            const int p = first(m_sync, bx1 + 21, xe - 38 + 1);
            if (p < 0) { a = xe; break; }
            a = (p + 38 > a1) ? p + 38 : a1;
            bx = (a - kBuf > bx) ? a - kBuf : bx;
            nfs = abs_of(p) + 296u;
            state = kKnowFstart;
        } else if (state == kKnowFstart) {
            const int nfs_x = x0 + (int)(int32_t)(nfs - abs0);
            const int at = (a + 1 > nfs_x) ? a + 1 : nfs_x;
            if (at > xe) { a = xe; break; }
            a = at;
            bx = nfs_x;
            nfs += kTs;
            state = kLocked;
            locked_call();
        } else {
            if (a == bx && xe - bx >= 2 * kTs) {
                bool unlocked = false;
                const int done = batch(bx, (xe - bx) / kTs, frames, abs_of(bx), unlocked);
                if (done > 0) {                                 // `done` LOCKED calls of exactly one frame each, a = bx + 510 after every one
                    frames += done;
                    bx += kTs * done;
                    nfs += (uint32_t)(kTs * done);
                    a = bx;
                    if (unlocked) state = kUnlocked;
                    continue;
                }
            }
            const int an = (a + 1 > bx + kTs) ? a + 1 : bx + kTs;
            if (an > xe) { a = xe; break; }
            a = an;
            bx = (a - kBuf > bx) ? a - kBuf : bx;
            locked_call();
        }
    }
    bx = (a - kBuf > bx) ? a - kBuf : bx;                       // make_bitbuf_space of the calls skipped at the end
    st.state = state;
    st.bits_in_buf = (uint32_t)(xe - bx);
    st.bitbuf_start_bitnum = abs_of(bx);
    st.next_frame_start_bitnum = nfs;
    carry_x = bx;
    return frames;
}

// walk() under the reference's rule, and under the tolerant one
template <class First, class Emit, class Batch>
BS_FN int run(State& st, const uint32_t* s, const uint32_t* m_sync, const uint32_t* m_n1, const uint32_t* m_n2, const uint32_t* m_any,
              int n_new, int& carry_x, First first, Emit emit, Batch batch) {
    RefLock lock{ m_sync, m_n1, m_n2, m_any };
    return walk(st, s, m_sync, n_new, carry_x, first, emit, batch, lock);
}
template <class First, class Emit, class Batch>
BS_FN int run_tolerant(State& st, const uint32_t* s, const uint32_t* m_sync, int n_new, int& carry_x, First first, Emit emit, Batch batch,
                       const Tolerance& tol, int& misses) {
    TolLock lock{ tol, misses };
    return walk(st, s, m_sync, n_new, carry_x, first, emit, batch, lock);
}

// ---- steps 1 and 4 of a channel's workgroup: the lane's share, thread tid of kThreads ----------------------------------------------------
constexpr int kThreads = 256;       // four wavefronts per channel for the byte work, one of them walks the state machine
constexpr int kFrameWords = 16, kFrameStride = 512;             // TETRA_FRAME_WORDS, TETRA_FRAME_STRIDE
struct FrameRec { int bx; int type; uint32_t bitnum; };         // a consumed frame, as emit() gets it

struct alignas(16) U4 { uint32_t x, y, z, w; };
BS_FN U4 load16(const uint8_t* p) {                             // p is 16-byte aligned
#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
    return *reinterpret_cast<const U4*>(p);
#else
    U4 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, 16), 16);
    return v;
#endif
}

// word w of the packed stream: the carried buffer cbuf (x0 .. kOff, one byte per bit) followed by n_new bytes of the row `in`; only bit
// 0 of a byte counts.  The new bits start word-aligned: 32 bytes -> one word with two 16-byte loads where the row's address allows them
// and one multiply per 8 bytes (the scan kernel's trick).
BS_FN uint32_t stream_word(int w, int x0, int n_new, const uint8_t* cbuf, const uint8_t* in) {
    uint32_t v = 0;
    const int xb = 32 * w;
    if (xb + 32 > x0 && xb < kOff) {                             // carried bits: byte by byte (at most 128 words)
        for (int b = 0; b < 32; ++b) {
            const int x = xb + b;
            if (x >= x0 && x < kOff) v |= (uint32_t)(cbuf[x - x0] & 1u) << (31 - b);
        }
    } else if (xb >= kOff && xb < kOff + n_new) {
        const int j = xb - kOff;
        if (j + 32 <= n_new && (((uintptr_t)(in + j)) & 15) == 0) {
            const U4 lo = load16(in + j), hi = load16(in + j + 16);
            const unsigned long long q[4] = { ((unsigned long long)lo.y << 32) | lo.x, ((unsigned long long)lo.w << 32) | lo.z,
                                              ((unsigned long long)hi.y << 32) | hi.x, ((unsigned long long)hi.w << 32) | hi.z };
#pragma unroll
            for (int z = 0; z < 4; ++z)      // 8 bytes -> 8 bits, first byte = MSB: byte i of x * 0x8040201008040201 reaches bit 63 - i
                v |= (uint32_t)(((q[z] & 0x0101010101010101ull) * 0x8040201008040201ull) >> 56) << (24 - 8 * z);
        } else {
            for (int b = 0; b < 32; ++b)
                if (j + b < n_new) v |= (uint32_t)(in[j + b] & 1u) << (31 - b);
        }
    }
    return v;
}
BS_FN void stage_thread(int tid, uint32_t* s, int words, int x0, int n_new, const uint8_t* cbuf, const uint8_t* in) {
    for (int w = tid; w < words; w += kThreads) s[w] = stream_word(w, x0, n_new, cbuf, in);
}

// word w of the packed frame that starts at bx (first bit = most significant; word 15 holds bits 480 .. 509 in its top 30 bits)
BS_FN uint32_t frame_word(const uint32_t* s, int bx, int w) {
    const uint32_t v = window(s, bx + 32 * w, 32);
    return w == kFrameWords - 1 ? v & 0xfffffffcu : v;          // bits 510, 511 of the row are not the frame's
}
// dword d of its byte form: four bits as four bytes, zero from bit 510 on
BS_FN uint32_t frame_dword(const uint32_t* s, int bx, int d) {
    uint32_t nib = window(s, bx + 4 * d, 4);                    // first bit = MSB
    if (4 * d + 4 > kTs) nib &= (4 * d >= kTs) ? 0u : (0xfu << (4 * d + 4 - kTs)) & 0xfu;
    return ((nib >> 3) & 1u) | (((nib >> 2) & 1u) << 8) | (((nib >> 1) & 1u) << 16) | ((nib & 1u) << 24);
}
// The channel's outputs from the frame list rec[0 .. nf) of the walk: frames ([max_frames][16] words, PACKED, or [max_frames][512]
// bytes), types and bit numbers of all max_frames slots (none_type behind the list), and the new carried buffer [carry_x, xe).
template <bool PACKED>
BS_FN void write_thread(int tid, const uint32_t* s, const FrameRec* rec, int nf, int max_frames, int none_type, int carry_x, int xe,
                        uint8_t* frames, int32_t* frame_type, uint32_t* frame_bitnum, uint8_t* cbuf) {
    if (PACKED) {
        uint32_t* pout = reinterpret_cast<uint32_t*>(frames);
        for (int i = tid; i < nf * kFrameWords; i += kThreads) pout[i] = frame_word(s, rec[i / kFrameWords].bx, i % kFrameWords);
    }
    for (int f = 0; !PACKED && f < nf; ++f) {
        const int bx = rec[f].bx;
        uint32_t* dst = reinterpret_cast<uint32_t*>(frames + (size_t)f * kFrameStride);
        for (int d = tid; d < kFrameStride / 4; d += kThreads) dst[d] = frame_dword(s, bx, d);
    }
    for (int f = tid; f < max_frames; f += kThreads) {
        frame_type[f] = f < nf ? rec[f].type : none_type;
        frame_bitnum[f] = f < nf ? rec[f].bitnum : 0u;
    }
    for (int i = tid; i < xe - carry_x; i += kThreads) cbuf[i] = (uint8_t)get_bit(s, carry_x + i);
}

}  // namespace bsync_core
