// Host build of the training-sequence search's and the indicator's lane code (sdrpp-tetra-demodulator_amd/csrc/scan_core.hpp) --
// the source the kernels compile -- walked as one workgroup of tetra_burst_scan.hip walks a channel: the pre-filter by thread 0,
// then tile by tile the packing of every word of the tile and every position of it, thread after thread where the kernel has
// them side by side, the minimum (maximum) where it has the LDS atomic, and the early exit between tiles.  Test infrastructure:
// tests/test_burst_scan.py holds it to the reference's own tetra_find_train_seq and to the restated indicator without a GPU.
#define TETRA_HOST_EMUL 1
#include <cstdint>
#include <vector>

#include "../../sdrpp-tetra-demodulator_amd/csrc/scan_core.hpp"

using namespace scan_core;

namespace {
// LDS is not zeroed between workgroups and the kernel owns no word past its array: what a position reads there is not the row's
constexpr unsigned kStale = 0xa5c3965au;
constexpr int kSlack = 8;
}  // namespace

// k_find_train_seq for n_channels workgroups.  tiles[c]: how many tiles channel c packed (the early exit's effect).
extern "C" void scan_emul_find(const uint8_t* bits, int n_channels, int bits_stride, const int32_t* end_of_in, uint32_t mask,
                               int32_t* type_out, int32_t* off_out, int32_t* tiles) {
    std::vector<unsigned> lds(kTileWords + kSlack, kStale);
    unsigned* packed = lds.data();
    for (int ch = 0; ch < n_channels; ch++) {
        unsigned best = kNone, heads[5];
        const uint8_t* in = bits + (long long)ch * bits_stride;
        const int end = clamp_end(end_of_in[ch], bits_stride);
        for (int t = 0; t < 5; t++) heads[t] = head22(t);
        if (end > 0) {
            unsigned filter = 0;
            for (int i = 0; i < 20; i++) filter = (filter << 1) | in[i];
            const int lim = end < kEarly ? end : kEarly;
            for (int cur = 0; cur < lim; cur++) {
                filter = prefilter_step(filter, in, cur);
                bool m = false;
                for (int s = 0; s < 5; s++) m |= (filter == heads[s]);
                if (m) {
                    const int s = verify(in, cur, end, mask);
                    if (s < 5) { best = match_key(cur, s); break; }
                }
            }
        }
        int walked = 0;
        for (int base = 0; base < end; base += kTile) {
            if (scan_done(best, base)) break;
            walked++;
            for (int t = 0; t < kThreads; t++)
                for (int w = t; w < kTileWords; w += kThreads) packed[w] = pack_word(in, base + 32 * w, bits_stride);
            const int lim = (end - base < kTile) ? (end - base) : kTile;
            for (int t = 0; t < kThreads; t++)
                for (int r = t; r < lim; r += kThreads) {
                    if (candidate(packed, heads, base, r)) {
                        const int s = verify(in, base + r, end, mask);
                        if (s < 5 && match_key(base + r, s) < best) best = match_key(base + r, s);
                    }
                }
        }
        if (best == kNone) { type_out[ch] = -1; off_out[ch] = -1; }
        else { type_out[ch] = c_type[best & 7u]; off_out[ch] = (int)(best >> 3); }
        if (tiles) tiles[ch] = walked;
    }
}

// k_ts_indicator for n_channels workgroups: tail [n_channels][44] and expire [n_channels] are the handle's carried state
extern "C" void scan_emul_indicator(const uint8_t* bits, int n_channels, int bits_stride, const int32_t* n_bits, uint8_t* tail,
                                    int32_t* expire, uint8_t* found_out, int32_t* expire_out) {
    std::vector<unsigned> lds(kIndTileWords + kSlack, kStale);
    unsigned* packed = lds.data();
    for (int ch = 0; ch < n_channels; ch++) {
        unsigned long long heads[8];
        uint8_t new_tail[kIndTail];
        int last_hit = -1;
        const uint8_t* in = bits + (long long)ch * bits_stride;
        uint8_t* tl = tail + (long long)ch * kIndTail;
        const int n = ind_clamp(n_bits[ch], bits_stride);
        for (int t = 0; t < 8; t++) heads[t] = ind_head(t);
        for (int base = 0; base < n; base += kIndTile) {
            for (int t = 0; t < kThreads; t++)
                for (int w = t; w < kIndTileWords; w += kThreads) packed[w] = ind_pack_word(tl, in, n, base + 32 * w);
            const int lim = (n - base < kIndTile) ? (n - base) : kIndTile;
            for (int t = 0; t < kThreads; t++) {
                int mine = -1;
                for (int r = t; r < lim; r += kThreads)
                    if (ind_hit(packed, heads, r)) mine = base + r;
                if (mine > last_hit) last_hit = mine;
            }
        }
        if (n > 0) {
            for (int t = 0; t < kIndTail; t++) new_tail[t] = (uint8_t)ind_vbit(tl, in, n, n + t);
            for (int t = 0; t < kIndTail; t++) tl[t] = new_tail[t];
        }
        int e = expire[ch];
        if (n > 0) {
            e = ind_expire(e, n, last_hit);
            expire[ch] = e;
        }
        found_out[ch] = e > 0 ? 1 : 0;
        if (expire_out) expire_out[ch] = e;
    }
}

// words packed per route since the last call, and loads the hardware could not have made: {16-byte, dword, byte, misaligned}
extern "C" void scan_emul_trace(int64_t* out, int reset) {
    Trace& t = trace();
    out[0] = t.route16; out[1] = t.route4; out[2] = t.route1; out[3] = t.misaligned;
    if (reset) t = Trace();
}

extern "C" int scan_emul_tile(void) { return kTile; }
extern "C" int scan_emul_ind_tile(void) { return kIndTile; }
