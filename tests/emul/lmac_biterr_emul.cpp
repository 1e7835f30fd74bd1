// Host build of the channel bit-error count (include/ext/tetra_biterr.h): reencode_errors of lmac_core.hpp behind the decoder's front
// ends -- what k_lmac_decode, k_lmac_frames and k_lmac_frames_soft run when a launch asks for counts.  Each entry is a loop over
// workgroups and lanes that picks the front end the kernel calls (lmac_core.hpp, soft_core.hpp; the cooperative stage of byte rows is
// lmac_lane_io.hpp's stage_workgroup) and runs lmac_lane_io.hpp's lane epilogue with a count function behind it.  Test infrastructure:
// lets the CPU suite hold the exact lane source against the reference's encoder primitives without a GPU.
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
    const BlockKind kind{ kLayoutNone, p.type345 };
    const uint32_t* seq_tab = route == 0 ? seq_table() : nullptr;
    int fast = 0;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        const uint8_t* rows = type5 + (size_t)blk0 * in_stride;
        uint32_t xb[kLanes][kSeqWords];
        const bool packed = stage_workgroup(seq_tab, p.type345, type5, rows, rows_here, in_stride, xb);
        if (packed) fast += rows_here;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            const uint32_t code = type == TETRA_TPSAP_T_SB1 ? kScrambInitSb1 : scramb_init[blk];
            uint32_t cls[kClsWords + 1];
            auto half = [&](int h) { return outw[h][lane]; };
            auto ld = [&](int w) { return cls[w]; };
            auto st = [&](int w, uint32_t word) { cls[w] = word; };
            if (packed) {
                descramble_words(p.type345, code, xb[lane], seq_rows(seq_tab), st);
                finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<true>(p.type345, p.type2, p.a, ld, io); },
                            [&](bool) { return bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld); }, NoRescue(), &crc_ok[blk], &biterr[blk], nullptr);
            } else {
                byte_row_block(&kind, code, row_words(rows + (size_t)lane * in_stride), st);
                finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<false>(p.type345, p.type2, p.a, ld, io); },
                            [&](bool) { return bit_errors_hard<false>(p.type345, p.type2, p.a, half, ld); }, NoRescue(), &crc_ok[blk], &biterr[blk], nullptr);
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
    const BlockKind kind{ layout, p.type345 };
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            const FrameRef fr = frame_of(tpsap, row_frame, blk, frame_scramb);
            uint32_t fw[kFrameWords], cls[kSeqWords];
            load_frame(frame_rows(frames, fr.f), fw);
            frame_hard_block(&kind, fr.code, fw, [&] { return frame_type[fr.f]; }, seq_rows(seq_table()), [&](int w, uint32_t word) { cls[w] = word; });
            auto ld = [&](int w) { return cls[w]; };
            finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<true>(p.type345, p.type2, p.a, ld, io); },
                        [&](bool) { return bit_errors_hard<true>(p.type345, p.type2, p.a, [&](int h) { return outw[h][lane]; }, ld); }, NoRescue(),
                        &crc_ok[blk], &biterr[blk], nullptr);
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
    const BlockKind kind{ layout, p.type345 };
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int j = blk0 + lane;
            uint32_t soft[kSoftWords] = {};
            soft_block(&kind, scramb ? scramb[j] : kScrambInitSb1, [&] { return bitnum[j]; }, [&] { return frame_type[j]; }, seq_rows(seq_table()),
                       ring_words(rings + (size_t)j * ring_size), ring_size / 4u, [&](int g, uint32_t word) { soft[g] = word; });
            auto ld = [&](int w) { return soft[w]; };
            finish_lane(outw, lane, [&](LaneIo& io) { return decode_soft(p.type345, p.type2, p.a, ld, io); },
                        [&](bool) { return bit_errors_soft(p.type345, p.type2, p.a, [&](int h) { return outw[h][lane]; }, ld); }, NoRescue(), &crc_ok[j],
                        &biterr[j], nullptr);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}
