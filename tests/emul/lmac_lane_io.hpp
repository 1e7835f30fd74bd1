// What the host emulations of the lower-MAC decoder (lmac_emul.cpp, lmac_biterr_emul.cpp, lmac_soft_emul.cpp, lmac_list_emul.cpp) put
// around the lane code where the kernels have LDS, global memory and barriers: a workgroup is a loop over 64 lanes, its shared arrays are
// plain arrays.  The accessors of the block front ends (lmac_core.hpp, soft_core.hpp), k_lmac_decode's cooperative stage for a
// workgroup, and the one lane epilogue -- decode, count, rescue, verdict -- that every entry of those files runs behind its front end.
#pragma once
#include <climits>
#include <cstdint>
#include <cstring>

#include "../../sdrpp-tetra-demodulator_amd/csrc/lmac_core.hpp"

namespace lane_emul {

using namespace tetra_lmac;

typedef uint16_t OutW[kMaxType2 / 16][kLanes];      // decoded halves, [half][lane]

// the `io` of decode_hard / decode_soft for one lane
struct LaneIo {
    OutW& outw;
    int lane;
    uint32_t dec[(kMaxType2 + kFlush) / 2];
    void dec_st(int u, uint32_t w) { dec[u] = w; }
    uint32_t dec_ld(int u) const { return dec[u]; }
    void out_st(int h, uint32_t half) { outw[h][lane] = (uint16_t)half; }
    uint32_t tinv(uint32_t off) const {
        static const CrcInvTable crci = make_crc_inv_table();
        return crci.t[off >> 2];
    }
};

// step 4 of a workgroup: every lane's share of write_rows, by the route the kernel would take for these rows
inline void write_rows(const OutW& outw, int rows_here, int type2, uint8_t* out0, int out_stride) {
    for (int lane = 0; lane < kLanes; ++lane)
        tetra_lmac::write_rows(lane, rows_here, type2, rows_wide(out0, out_stride), [&](int h, int q) { return outw[h][q]; },
                               [&](int q, int d, demux_core::U2 v) { std::memcpy(out0 + (size_t)q * out_stride + 8 * d, &v, 8); },
                               [&](int q, int d, uint32_t v) { std::memcpy(out0 + (size_t)q * out_stride + 4 * d, &v, 4); });
}

// lane_sequence's rows of a host table [4][256][kSeqStride]
inline auto seq_rows(const uint32_t* tab) {
    return [=](int t, uint32_t byte) { return reinterpret_cast<const U4*>(tab + ((size_t)t * 256 + byte) * kSeqStride); };
}
inline const uint32_t* seq_table() {
    static uint32_t* tab = nullptr;
    if (!tab) {
        tab = new uint32_t[(size_t)4 * 256 * kSeqStride];
        scramb_sequence_table(tab);
    }
    return tab;
}
// load_frame's 16-byte rows of frame f, byte_row_block's words of a byte row (any alignment), soft_block's words of a ring
inline auto frame_rows(const uint32_t* frames, int f) {
    return [=](int g) { U4 v; std::memcpy(&v, frames + (size_t)f * kFrameWords + 4 * g, 16); return v; };
}
inline auto row_words(const uint8_t* row) {
    return [=](int d) { uint32_t v; std::memcpy(&v, row + 4 * d, 4); return v; };
}
inline auto ring_words(const int8_t* ring) {
    return [=](uint32_t w) { return reinterpret_cast<const uint32_t*>(ring)[w]; };
}
// A listed row's frame and code as the kernels look them up.  (The entries here take no frame count: their callers list frames that
// exist.  SB1 has its fixed code whatever the caller hands in, as the host side of the decoder passes no codes for it.)
inline FrameRef frame_of(int tpsap, const int32_t* row_frame, int row, const uint32_t* frame_scramb) {
    return frame_lookup(row_frame[row], INT_MAX, tpsap == TETRA_TPSAP_T_SB1 ? nullptr : frame_scramb);
}

// k_lmac_decode's cooperative front end for one workgroup: rows_here rows from `rows` on, type5 / in_stride the whole batch's.  True: the
// packed route is taken and xb[lane] holds the lane's packed row; false: the whole workgroup has to take the byte route.  The staging
// array starts out as all ones: the kernel's LDS is not cleared, and what staged_row lets through of that must not matter.
inline bool stage_workgroup(const uint32_t* seq_tab, int type345, const uint8_t* type5, const uint8_t* rows, int rows_here, int in_stride,
                            uint32_t xb[kLanes][kSeqWords]) {
    if (needs_byte_route(seq_tab, type5, in_stride)) return false;
    uint32_t stage[kLanes][kStageWords];
    std::memset(stage, 0xff, sizeof(stage));
    uint8_t* sb = reinterpret_cast<uint8_t*>(&stage[0][0]);
    uint32_t dirty = 0;                                           // the kernel's ballot
    for (int lane = 0; lane < kLanes; ++lane)
        dirty |= pack_units(lane, rows_here, in_stride, type345, [&](int u) { U2 d; std::memcpy(&d, rows + (size_t)8 * u, 8); return d; },
                            [&](size_t at, uint8_t byte) { sb[at] = byte; });
    if (dirty) return false;
    for (int lane = 0; lane < rows_here; ++lane) staged_row(type345, [&](int w) { return stage[lane][w]; }, xb[lane]);
    return true;
}

// The lane behind its front end, what a decode kernel and the rescue launch behind it leave of one row:
//   decode(io) -> whether the CRC is good, the decoded halves in the lane's column of outw;
//   count(rescued) -> the channel bit errors of the column against the staged block, asked for when `biterr` is given: once behind the
//     decoder, and again behind a rescue that won (rescued = true: the rescue kernel counts on ITS staging of the block);
//   rescue(io) -> the rank (list_core.hpp), asked for when `rank` is given and the CRC failed; a row nothing rescues keeps the decoder's
//     bits, so the column is saved around it;
//   the verdict.
// crc_ok, biterr, rank: the row's entries; biterr and rank may be NULL.
struct NoRescue { int operator()(LaneIo&) const { return -1; } };
template <class Decode, class Count, class Rescue>
inline void finish_lane(OutW& outw, int lane, Decode decode, Count count, Rescue rescue, int32_t* crc_ok, uint32_t* biterr, int32_t* rank) {
    LaneIo io{ outw, lane, {} };
    bool good = decode(io);
    if (biterr) *biterr = count(false);
    if (rank) {
        *rank = 0;
        if (!good) {
            uint16_t saved[kMaxType2 / 16];
            for (int i = 0; i < kMaxType2 / 16; ++i) saved[i] = outw[i][lane];
            *rank = rescue(io);
            if (*rank > 0) {
                good = true;
                if (biterr) *biterr = count(true);
            } else {
                for (int i = 0; i < kMaxType2 / 16; ++i) outw[i][lane] = saved[i];
            }
        }
    }
    *crc_ok = good;
}

}  // namespace lane_emul
