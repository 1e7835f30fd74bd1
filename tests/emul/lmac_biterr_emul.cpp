// Host build of the channel bit-error count (include/ext/tetra_biterr.h): reencode_errors of lmac_core.hpp behind the decoder's three front
// ends, a 64-row workgroup at a time with plain arrays where the kernels have LDS (lmac_lane_io.hpp) -- what k_lmac_decode,
// k_lmac_frames and k_lmac_frames_soft run when a launch asks for counts.  Test infrastructure: lets the CPU suite hold the exact lane
// source against the reference's encoder primitives without a GPU.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/soft_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_soft;
using namespace lane_emul;

// k_lmac_decode with counts.  route: 0 = like the kernel (a workgroup whose rows are all plain bits, 8-byte aligned and at most 512 bytes
// apart takes the packed route, any other the byte route), 1 = byte route always.  biterr [n_blocks]: errors | compared << 16;
// fast_rows: the rows of the workgroups that took the packed route.
extern "C" int biterr_emul_rows(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                                int32_t* crc_ok, uint32_t* biterr, int route, int32_t* fast_rows) {
    if (type < 0 || type > 5 || type == TETRA_TPSAP_T_BBK || (in_stride & 3)) return -1;
    const BlkParam& p = blk_param(type);
    const uint32_t* seq_tab = route == 0 ? seq_table() : nullptr;
    int fast = 0;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        const uint8_t* rows = type5 + (size_t)blk0 * in_stride;
        // the cooperative front end (the staging array starts out as all ones: the kernel's LDS is not cleared)
        bool packed = !needs_byte_route(seq_tab, type5, in_stride);
        uint32_t stage[kLanes][kStageWords];
        std::memset(stage, 0xff, sizeof(stage));
        if (packed) {
            uint8_t* sb = reinterpret_cast<uint8_t*>(&stage[0][0]);
            uint32_t dirty = 0;
            for (int lane = 0; lane < kLanes; ++lane)
                dirty |= pack_units(lane, rows_here, in_stride, p.type345, [&](int u) { U2 d; std::memcpy(&d, rows + (size_t)8 * u, 8); return d; },
                                    [&](size_t at, uint8_t byte) { sb[at] = byte; });
            packed = dirty == 0;
        }
        if (packed) fast += rows_here;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const uint32_t code = type == TETRA_TPSAP_T_SB1 ? kScrambInitSb1 : scramb_init[blk0 + lane];
            uint32_t cls[kClsWords + 1];
            LaneIo io{ outw, lane, {} };
            auto half = [&](int h) { return outw[h][lane]; };
            auto ld = [&](int w) { return cls[w]; };
            if (packed) {
                uint32_t xb[kSeqWords];
                staged_row(p.type345, [&](int w) { return stage[lane][w]; }, xb);
                descramble_words(p.type345, code, xb, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w] = word; });
                crc_ok[blk0 + lane] = decode_hard<true>(p.type345, p.type2, p.a, ld, io);
                biterr[blk0 + lane] = bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld);
            } else {
                const uint8_t* row = rows + (size_t)lane * in_stride;
                uint32_t lfsr = code;
                for (int c0 = 0; c0 < p.type345 / 4; c0 += kChunkDwords)      // the kernel's 64-bit staging chunks
                    lfsr = descramble_chunk(p.type345 - 4 * c0, lfsr, [&](int d) { uint32_t v; std::memcpy(&v, row + 4 * (c0 + d), 4); return v; },
                                            [&](int w, uint32_t word) { cls[c0 / 4 + w] = word; });
                crc_ok[blk0 + lane] = decode_hard<false>(p.type345, p.type2, p.a, ld, io);
                biterr[blk0 + lane] = bit_errors_hard<false>(p.type345, p.type2, p.a, half, ld);
            }
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    if (fast_rows) *fast_rows = fast;
    return 0;
}

// k_lmac_frames with counts, one job of a coded kind: the listed frames (frames [n_frames][16] packed, frame_scramb per frame slot,
// NULL: SCRAMB_INIT).
extern "C" int biterr_emul_frames(int tpsap, int blk_num, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame, int n_rows,
                                  const uint32_t* frame_scramb, uint8_t* out, int out_stride, int32_t* crc_ok, uint32_t* biterr) {
    const int layout = tpsap < 0 || tpsap > 5 || tpsap == TETRA_TPSAP_T_BBK ? kLayoutNone : layout_for(tpsap, blk_num, false);
    if (layout == kLayoutNone) return -1;
    const BlkParam& p = blk_param(tpsap);
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane, f = row_frame[blk];
            const uint32_t code = frame_scramb && tpsap != TETRA_TPSAP_T_SB1 ? frame_scramb[f] : kScrambInitSb1;
            uint32_t xb[kSeqWords], cls[kSeqWords];
            frame_block(layout, frames + (size_t)f * kFrameWords, frame_type[f], xb);
            descramble_words(p.type345, code, xb, seq_rows(seq_table()), [&](int w, uint32_t word) { cls[w] = word; });
            LaneIo io{ outw, lane, {} };
            auto ld = [&](int w) { return cls[w]; };
            crc_ok[blk] = decode_hard<true>(p.type345, p.type2, p.a, ld, io);
            biterr[blk] = bit_errors_hard<true>(p.type345, p.type2, p.a, [&](int h) { return outw[h][lane]; }, ld);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}

// k_lmac_frames_soft with counts, a lane per row: arguments as soft_emul_decode (lmac_soft_emul.cpp) plus biterr [n_rows].
extern "C" int biterr_emul_soft(int tpsap, int blk_num, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type,
                                int n_rows, const uint32_t* scramb, uint8_t* out, int out_stride, int32_t* crc_ok, uint32_t* biterr) {
    const int layout = tpsap < 0 || tpsap > 5 || tpsap == TETRA_TPSAP_T_BBK ? kLayoutNone : layout_for(tpsap, blk_num, false);
    if (layout == kLayoutNone || ring_size < 4 || (ring_size & (ring_size - 1))) return -1;
    const BlkParam& p = blk_param(tpsap);
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int j = blk0 + lane;
            const uint32_t* ring = reinterpret_cast<const uint32_t*>(rings + (size_t)j * ring_size);
            uint32_t seq[kSeqWords] = {}, soft[kSoftWords] = {};
            lane_sequence(p.type345, scramb ? scramb[j] : kScrambInitSb1, seq_rows(seq_table()), [&](int w, uint32_t word) { seq[w] = word; });
            stage_block(layout, bitnum[j], frame_type[j], [&](uint32_t w) { return ring[w]; }, ring_size - 1u, seq, [&](int g, uint32_t word) { soft[g] = word; });
            LaneIo io{ outw, lane, {} };
            auto ld = [&](int w) { return soft[w]; };
            crc_ok[j] = decode_soft(p.type345, p.type2, p.a, ld, io);
            biterr[j] = bit_errors_soft(p.type345, p.type2, p.a, [&](int h) { return outw[h][lane]; }, ld);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}
