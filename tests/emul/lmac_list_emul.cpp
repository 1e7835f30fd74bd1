// Host build of the CRC-aided list decoding (include/ext/tetra_list.h): list_core.hpp behind the decoder's front ends -- what a decode
// launch with ranks and the k_list_rescue launch behind it compute together.  Each entry is a loop over workgroups and lanes that picks
// the front end the kernels call (lmac_core.hpp, soft_core.hpp; the cooperative stage of byte rows is lmac_lane_io.hpp's
// stage_workgroup) and runs lmac_lane_io.hpp's lane epilogue with a rescue function behind it.  Test infrastructure: lets the CPU suite
// hold the exact lane source against an independent statement of the definition without a GPU.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/list_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_soft;
using namespace lane_emul;

// k_lmac_decode + k_list_rescue<bytes>.  route: as biterr_emul_rows' (0 = like the kernel, 1 = byte route always).  The rescue stages the
// row through the byte route as the kernel does; bits_rescue != 0 stages plain rows (every byte 0 / 1) as packed bits instead, the
// decode launch's packed route: the same margins.  biterr may be NULL.
extern "C" int list_emul_rows(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                              int32_t* crc_ok, int32_t* rank, uint32_t* biterr, int route, int max_candidates, int bits_rescue) {
    if (type < 0 || type > 5 || type == TETRA_TPSAP_T_BBK || (in_stride & 3) || max_candidates < 1 || max_candidates > tetra_list::kMaxCandidates) return -1;
    const BlkParam& p = blk_param(type);
    const BlockKind kind{ kLayoutNone, p.type345 };
    const uint32_t* seq_tab = route == 0 ? seq_table() : nullptr;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        const uint8_t* rows = type5 + (size_t)blk0 * in_stride;
        uint32_t xb[kLanes][kSeqWords];
        const bool packed = stage_workgroup(seq_tab, p.type345, type5, rows, rows_here, in_stride, xb);
        if (bits_rescue && !packed) return -2;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            const uint32_t code = type == TETRA_TPSAP_T_SB1 ? kScrambInitSb1 : scramb_init[blk];
            uint32_t bits[kSeqWords] = {}, cls[kClsWords + 1] = {};
            auto half = [&](int h) { return outw[h][lane]; };
            auto ld_bits = [&](int w) { return bits[w]; };
            auto ld_cls = [&](int w) { return cls[w]; };
            byte_row_block(&kind, code, row_words(rows + (size_t)lane * in_stride), [&](int w, uint32_t word) { cls[w] = word; });      // the rescue's staging
            if (packed) descramble_words(p.type345, code, xb[lane], seq_rows(seq_tab), [&](int w, uint32_t word) { bits[w] = word; });
            finish_lane(outw, lane,
                        [&](LaneIo& io) { return packed ? decode_hard<true>(p.type345, p.type2, p.a, ld_bits, io) : decode_hard<false>(p.type345, p.type2, p.a, ld_cls, io); },
                        [&](bool rescued) {
                            return packed && !rescued ? bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld_bits) : bit_errors_hard<false>(p.type345, p.type2, p.a, half, ld_cls);
                        },
                        [&](LaneIo& io) {
                            return bits_rescue ? tetra_list::rescue_hard<true>(p.type345, p.type2, p.a, max_candidates, ld_bits, io, half)
                                               : tetra_list::rescue_hard<false>(p.type345, p.type2, p.a, max_candidates, ld_cls, io, half);
                        },
                        &crc_ok[blk], biterr ? &biterr[blk] : nullptr, &rank[blk]);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}

// k_lmac_frames + k_list_rescue<frames>, one job of a coded kind (arguments as biterr_emul_frames; biterr may be NULL)
extern "C" int list_emul_frames(int tpsap, int blk_num, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame, int n_rows,
                                const uint32_t* frame_scramb, uint8_t* out, int out_stride, int32_t* crc_ok, int32_t* rank, uint32_t* biterr,
                                int max_candidates) {
    const int layout = tpsap < 0 || tpsap > 5 || tpsap == TETRA_TPSAP_T_BBK ? kLayoutNone : layout_for(tpsap, blk_num, false);
    if (layout == kLayoutNone || max_candidates < 1 || max_candidates > tetra_list::kMaxCandidates) return -1;
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
            auto half = [&](int h) { return outw[h][lane]; };
            finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<true>(p.type345, p.type2, p.a, ld, io); },
                        [&](bool) { return bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld); },
                        [&](LaneIo& io) { return tetra_list::rescue_hard<true>(p.type345, p.type2, p.a, max_candidates, ld, io, half); },
                        &crc_ok[blk], biterr ? &biterr[blk] : nullptr, &rank[blk]);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}

// k_lmac_frames_soft + k_list_rescue<soft>, a lane per row (arguments as biterr_emul_soft; biterr may be NULL)
extern "C" int list_emul_soft(int tpsap, int blk_num, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type,
                              int n_rows, const uint32_t* scramb, uint8_t* out, int out_stride, int32_t* crc_ok, int32_t* rank, uint32_t* biterr,
                              int max_candidates) {
    const int layout = tpsap < 0 || tpsap > 5 || tpsap == TETRA_TPSAP_T_BBK ? kLayoutNone : layout_for(tpsap, blk_num, false);
    if (layout == kLayoutNone || ring_size < 4 || (ring_size & (ring_size - 1)) || max_candidates < 1 || max_candidates > tetra_list::kMaxCandidates) return -1;
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
            auto half = [&](int h) { return outw[h][lane]; };
            finish_lane(outw, lane, [&](LaneIo& io) { return decode_soft(p.type345, p.type2, p.a, ld, io); },
                        [&](bool) { return bit_errors_soft(p.type345, p.type2, p.a, half, ld); },
                        [&](LaneIo& io) { return tetra_list::rescue_soft(p.type345, p.type2, p.a, max_candidates, ld, io, half); },
                        &crc_ok[j], biterr ? &biterr[j] : nullptr, &rank[j]);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}
