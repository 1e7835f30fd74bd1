// scan_core.hpp -- the lane-level code of the training-sequence search and of the plugin's indicator
// (include/tetra_burst_scan.h), shared by the gfx950 kernels (tetra_burst_scan.hip) and their host build
// (tests/emul/scan_emul.cpp, -DTETRA_HOST_EMUL).
//
// Everything that can be wrong per word or per position lives here: the byte -> bit packing with its three routes and the
// decision between them, the window pulls, the sequence tables and heads, the full check, the pre-filter of the first 21
// positions, the clamps, the early exit's condition and the indicator's counter arithmetic.  The kernels keep the loops over
// tiles, words and positions, the barriers and the LDS atomics; the host build walks the same loops one thread after the other.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define SC_FN __device__ __forceinline__
#define SC_TABLE static __constant__
#define SC_TRACE(field) ((void)0)
#else
#include <string.h>
#define SC_FN static inline
#define SC_TABLE static const
#define SC_TRACE(field) (++scan_core::trace().field)
#endif

namespace scan_core {

constexpr int kThreads = 256;
constexpr unsigned kNone = 0xffffffffu;      // "no match yet" in the (position << 3 | check order) key

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
typedef uint4 Vec4;
SC_FN Vec4 load16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }
SC_FN unsigned load4(const uint8_t* p) { return *reinterpret_cast<const unsigned*>(p); }
#else
// Host build: the same loads, counted per route, and a load that the hardware could not make as one access is counted too.
struct Trace { long long route16, route4, route1, misaligned; };
static inline Trace& trace() { static Trace t; return t; }
struct Vec4 { uint32_t x, y, z, w; };
static inline Vec4 load16(const uint8_t* p) {
    if (reinterpret_cast<uintptr_t>(p) & 15) SC_TRACE(misaligned);
    Vec4 v;
    memcpy(&v, p, 16);
    return v;
}
static inline unsigned load4(const uint8_t* p) {
    if (reinterpret_cast<uintptr_t>(p) & 3) SC_TRACE(misaligned);
    unsigned v;
    memcpy(&v, p, 4);
    return v;
}
#endif

// 8 bytes (one bit each) -> 8 bits, first byte = MSB, with one multiply: the partial products of x * 0x8040201008040201 land on
// distinct bit positions, byte i reaching bit 63 - i.
SC_FN unsigned pack8(unsigned long long q) { return (unsigned)(((q & 0x0101010101010101ull) * 0x8040201008040201ull) >> 56); }

// 32 bytes as four little-endian 64-bit words -> 32 bits, first byte = MSB
SC_FN unsigned pack32(const unsigned long long* q) {
    unsigned v = 0;
    for (int z = 0; z < 4; z++) v |= pack8(q[z]) << (24 - 8 * z);
    return v;
}

// 32 bytes at p, 16-byte aligned, as two 16-byte loads
SC_FN void load32_vec(const uint8_t* p, unsigned long long* q) {
    const Vec4 lo = load16(p), hi = load16(p + 16);
    q[0] = ((unsigned long long)lo.y << 32) | lo.x; q[1] = ((unsigned long long)lo.w << 32) | lo.z;
    q[2] = ((unsigned long long)hi.y << 32) | hi.x; q[3] = ((unsigned long long)hi.w << 32) | hi.z;
}

// 32 bytes at p, 4-byte aligned, as dword loads
SC_FN void load32_dword(const uint8_t* p, unsigned long long* q) {
    for (int z = 0; z < 4; z++) q[z] = ((unsigned long long)load4(p + 8 * z + 4) << 32) | load4(p + 8 * z);
}

// =====================================================================================================================
// The search: tetra_find_train_seq(), src/decoder/src/phy/tetra_burst.c:271-341
// =====================================================================================================================
constexpr int kTile = 32768;                 // positions per tile
constexpr int kTileWords = kTile / 32 + 2;   // + look-ahead: a position's 22-bit window reaches into the word after its own
constexpr int kEarly = 21;                   // positions 0..20 see the reference's misaligned pre-filter

// ETSI EN 300 392-2 9.4.4.3.2-4 (the reference holds the same bits at tetra_burst.c:61-72)
SC_TABLE uint8_t c_seq[5][38] = {
    /* check order of the reference's if-chain: y (sync), n, p, q (normal 1-3), x (extended) */
    { 1,1, 0,0, 0,0, 0,1, 1,0, 0,1, 1,1, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,0, 0,0, 0,1, 1,0, 0,1, 1,1 },
    { 1,1, 0,1, 0,0, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,1, 0,0 },
    { 0,1, 1,1, 1,0, 1,0, 0,1, 0,0, 0,0, 1,1, 0,1, 1,1, 1,0 },
    { 1,0, 1,1, 0,1, 1,1, 0,0, 0,0, 0,1, 1,0, 1,0, 1,1, 0,1 },
    { 1,0, 0,1, 1,1, 0,1, 0,0, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,1, 0,0, 0,0, 1,1 },
};
SC_TABLE int c_len[5] = { 38, 22, 22, 22, 30 };
// enum tetra_train_seq (tetra_burst.h:26-32 = TETRA_TRAIN_x of tetra_burst_scan.h): SYNC, NORM_1, NORM_2, NORM_3, EXT
SC_TABLE int c_type[5] = { 3, 0, 1, 2, 4 };

SC_FN unsigned head22(int s) {
    unsigned v = 0;
    for (int i = 0; i < 22; i++) v = (v << 1) | c_seq[s][i];
    return v;
}

SC_FN unsigned match_key(int cur, int s) { return ((unsigned)cur << 3) | (unsigned)s; }

// the search reads in[cur + 21] for every cur < end (tetra_burst.c:296): a count that would take that look-ahead out of
// the row is cut back to what the row holds (documented in tetra_burst_scan.h: rows extend 21 bytes past end_of_in)
SC_FN int clamp_end(int end, int bits_stride) { return end > bits_stride - 21 ? bits_stride - 21 : end; }

// full check of the reference's if-chain at position cur; returns the check-order index 0..4 or 5 for none
SC_FN int verify(const uint8_t* in, int cur, int end_of_in, unsigned mask) {
    const int remain = end_of_in - cur;
    for (int s = 0; s < 5; s++) {
        if (!(mask & (1u << c_type[s])) || remain < c_len[s]) continue;
        bool eq = true;
        for (int i = 0; i < c_len[s]; i++)
            if (in[cur + i] != c_seq[s][i]) { eq = false; break; }
        if (eq) return s;
    }
    return 5;
}

// positions 0..20: the reference's pre-filter is seeded with in[0..19] and then receives in[cur+21] (in[20] is skipped).  One
// thread walks cur = 0 .. min(end, kEarly) - 1 in order, stepping the filter once per position, and stops at the first position
// whose filter fires AND whose full check succeeds.  (The seed loop stays in the callers: as a function of this header it costs
// the kernel time, profiles/HISTORY.md; the five-head compare stays beside it.)
SC_FN unsigned prefilter_step(unsigned filter, const uint8_t* in, int cur) { return ((filter << 1) | in[cur + 21]) & 0x3fffffu; }

// before the tile that starts at `base`: an earlier match ends the scan
SC_FN bool scan_done(unsigned best, int base) { return best != kNone && (int)(best >> 3) < base; }

// Word w of a tile: bytes [b0, b0 + 32) of the row -> 32 bits, MSB first; bytes past the row are taken as 0 (never reached by
// a position < end whose 22-bit window lies inside end + 21 <= bits_stride).  Three routes: two 16-byte loads where the
// ADDRESS is 16-byte aligned (the entry point accepts any 4-byte aligned base, so the stride alone does not say), dword loads
// otherwise (rows are 4-byte aligned), byte by byte for the word that hangs over the end of the row.
SC_FN unsigned pack_word(const uint8_t* in, int b0, int bits_stride) {
    unsigned v = 0;
    if (b0 + 32 <= bits_stride) {
        unsigned long long q[4];
        if (((reinterpret_cast<uintptr_t>(in) | (unsigned)b0) & 15) == 0) {
            SC_TRACE(route16);
            load32_vec(in + b0, q);
        } else {
            SC_TRACE(route4);
            load32_dword(in + b0, q);
        }
        v = pack32(q);
    } else {
        SC_TRACE(route1);
        for (int z = 0; z < 32; z++)
            if (b0 + z < bits_stride) v |= (unsigned)(in[b0 + z] & 1u) << (31 - z);
    }
    return v;
}

// the 22 bits that start sh bits into word w0 (sh = 0..31), first bit most significant
SC_FN unsigned window22(unsigned w0, unsigned w1, int sh) {
    const unsigned long long two = ((unsigned long long)w0 << 32) | w1;
    return (unsigned)(two >> (64 - 22 - sh)) & 0x3fffffu;
}

// position r of the tile that starts at base (packed = that tile's words): does its 22-bit window hold one of the five heads,
// i.e. is it worth the full check
SC_FN bool candidate(const unsigned* packed, const unsigned* heads, int base, int r) {
    if (base + r < kEarly) return false;                             // handled by the pre-filter
    const unsigned f = window22(packed[r >> 5], packed[(r >> 5) + 1], r & 31);
    return f == heads[0] || f == heads[1] || f == heads[2] || f == heads[3] || f == heads[4];
}

// =====================================================================================================================
// The plugin's indicator: _demodSinkHandler, src/main.cpp:385-414
// =====================================================================================================================
constexpr int kIndWin = 45, kIndTail = kIndWin - 1, kIndArm = 2048;
constexpr int kIndTile = 8192, kIndTileWords = kIndTile / 32 + 3;     // a 45-bit window reaches two words past its own

// main.cpp:457-468, in the order of the if-chain at :395-402 (the order does not matter: any hit arms the counter)
SC_TABLE uint8_t c_ind_seq[8][45] = {
    { 1,1, 0,1, 0,0, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,1, 0,0 },
    { 0,1, 1,1, 1,0, 1,0, 0,1, 0,0, 0,0, 1,1, 0,1, 1,1, 1,0 },
    { 1,0, 1,1, 0,1, 1,1, 0,0, 0,0, 0,1, 1,0, 1,0, 1,1, 0,1 },
    { 1,1,1, 0,0,1, 1,0,1, 1,1,1, 0,0,0, 1,1,1, 1,0,0, 0,1,1, 1,1,0, 0,0,0, 0,0,0 },
    { 1,0,1, 0,1,1, 1,1,1, 1,0,1, 0,1,0, 1,0,1, 1,1,0, 0,0,1, 1,0,0, 0,1,0, 0,1,0 },
    { 1,0, 0,1, 1,1, 0,1, 0,0, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,1, 0,0, 0,0, 1,1 },
    { 0,1,1,1,0,0,1,1,0,1,0,0,0,0,1,0,0,0,1,1,1,0,1,1,0,1,0,1,0,1,1,1,1,1,0,1,0,0,0,0,0,1,1,1,0 },
    { 1,1, 0,0, 0,0, 0,1, 1,0, 0,1, 1,1, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,0, 0,0, 0,1, 1,0, 0,1, 1,1 },
};
SC_TABLE int c_ind_len[8] = { 22, 22, 22, 33, 33, 30, 45, 38 };

// sequence s as a number, first bit most significant: what the top c_ind_len[s] bits of a 45-bit window are compared with
SC_FN unsigned long long ind_head(int s) {
    unsigned long long v = 0;
    for (int i = 0; i < c_ind_len[s]; i++) v = (v << 1) | c_ind_seq[s][i];
    return v;
}

SC_FN int ind_clamp(int n, int bits_stride) { return n < 0 ? 0 : (n > bits_stride ? bits_stride : n); }

// v[i] = i < 44 ? carried bit i : bits[i - 44]; position q (the window after bit q of the call) covers v[q .. q + 44]
SC_FN unsigned ind_vbit(const uint8_t* tl, const uint8_t* in, int n, int i) {
    return i < kIndTail ? (tl[i] & 1u) : (i - kIndTail < n ? (in[i - kIndTail] & 1u) : 0u);
}

// v[b0 .. b0 + 32) -> 32 bits, MSB first: dword loads where all 32 lie in this call's bits, bit by bit at both ends
SC_FN unsigned ind_pack_word(const uint8_t* tl, const uint8_t* in, int n, int b0) {
    unsigned v = 0;
    if (b0 >= kIndTail + 4 && b0 - kIndTail + 32 <= n) {
        SC_TRACE(route4);
        unsigned long long q[4];
        load32_dword(in + (b0 - kIndTail), q);                        // 44 % 4 == 0: dword aligned
        v = pack32(q);
    } else {
        SC_TRACE(route1);
        for (int z = 0; z < 32; z++) v |= ind_vbit(tl, in, n, b0 + z) << (31 - z);
    }
    return v;
}

// the 45 bits that start sh bits into word w0 (sh = 0..31), first bit most significant
SC_FN unsigned long long window45(unsigned w0, unsigned w1, unsigned w2, int sh) {
    const unsigned long long hi = ((unsigned long long)w0 << 32) | w1;
    const unsigned long long top = sh ? ((hi << sh) | ((unsigned long long)w2 >> (32 - sh))) : hi;
    return top >> (64 - kIndWin);
}

// position r of a tile (packed = that tile's words): does the window's head hold one of the eight sequences
SC_FN bool ind_hit(const unsigned* packed, const unsigned long long* heads, int r) {
    const unsigned long long win = window45(packed[r >> 5], packed[(r >> 5) + 1], packed[(r >> 5) + 2], r & 31);
    bool hit = false;
    for (int s = 0; s < 8; s++) hit |= (win >> (kIndWin - c_ind_len[s])) == heads[s];
    return hit;
}

// symsbeforeexpire after a call of n > 0 bits whose last hit was at bit last_hit (or -1), carried in as e: a hit at bit p arms
// 2048 and the same bit counts it down to 2047; every later bit takes one more
SC_FN int ind_expire(int e, int n, int last_hit) {
    if (last_hit >= 0) e = kIndArm - 1 - (n - 1 - last_hit);
    else e = e - n;
    return e < 0 ? 0 : e;
}

}  // namespace scan_core
