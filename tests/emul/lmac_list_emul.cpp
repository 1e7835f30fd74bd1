// Host build of the CRC-aided list decoding (include/ext/tetra_list.h): list_core.hpp behind the decoder's three front ends, a 64-row
// workgroup at a time with plain arrays where the kernels have LDS (lmac_lane_io.hpp) -- what a decode launch with ranks and the
// k_list_rescue launch behind it compute together.  Test infrastructure: lets the CPU suite hold the exact lane source against an
// independent statement of the definition without a GPU.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/list_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_soft;
using namespace lane_emul;

namespace {

// the lane's decoded halves, saved so that a row nothing rescues keeps the decoder's bits
struct Column {
    uint16_t h[kMaxType2 / 16];
    void save(const OutW& outw, int lane) { for (int i = 0; i < kMaxType2 / 16; ++i) h[i] = outw[i][lane]; }
    void restore(OutW& outw, int lane) const { for (int i = 0; i < kMaxType2 / 16; ++i) outw[i][lane] = h[i]; }
};

}  // namespace

// k_lmac_decode + k_list_rescue<bytes>.  route: as biterr_emul_rows' (0 = like the kernel, 1 = byte route always).  The rescue stages the
// row through the byte route as the kernel does; bits_rescue != 0 stages plain rows (every byte 0 / 1) as packed bits instead, the
// decode launch's packed route: the same margins.  biterr may be NULL.
extern "C" int list_emul_rows(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                              int32_t* crc_ok, int32_t* rank, uint32_t* biterr, int route, int max_candidates, int bits_rescue) {
    if (type < 0 || type > 5 || type == TETRA_TPSAP_T_BBK || (in_stride & 3) || max_candidates < 1 || max_candidates > tetra_list::kMaxCandidates) return -1;
    const BlkParam& p = blk_param(type);
    const uint32_t* seq_tab = route == 0 ? seq_table() : nullptr;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        const uint8_t* rows = type5 + (size_t)blk0 * in_stride;
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
        if (bits_rescue && !packed) return -2;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            const uint32_t code = type == TETRA_TPSAP_T_SB1 ? kScrambInitSb1 : scramb_init[blk];
            uint32_t bits[kSeqWords] = {}, cls[kClsWords + 1] = {};
            LaneIo io{ outw, lane, {} };
            auto half = [&](int h) { return outw[h][lane]; };
            auto ld_bits = [&](int w) { return bits[w]; };
            auto ld_cls = [&](int w) { return cls[w]; };
            const uint8_t* row = rows + (size_t)lane * in_stride;
            uint32_t lfsr = code;
            for (int c0 = 0; c0 < p.type345 / 4; c0 += kChunkDwords)
                lfsr = descramble_chunk(p.type345 - 4 * c0, lfsr, [&](int d) { uint32_t v; std::memcpy(&v, row + 4 * (c0 + d), 4); return v; },
                                        [&](int w, uint32_t word) { cls[c0 / 4 + w] = word; });
            bool good;
            if (packed) {
                uint32_t xb[kSeqWords];
                staged_row(p.type345, [&](int w) { return stage[lane][w]; }, xb);
                descramble_words(p.type345, code, xb, seq_rows(seq_tab), [&](int w, uint32_t word) { bits[w] = word; });
                good = decode_hard<true>(p.type345, p.type2, p.a, ld_bits, io);
                if (biterr) biterr[blk] = bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld_bits);
            } else {
                good = decode_hard<false>(p.type345, p.type2, p.a, ld_cls, io);
                if (biterr) biterr[blk] = bit_errors_hard<false>(p.type345, p.type2, p.a, half, ld_cls);
            }
            rank[blk] = 0;
            if (!good) {
                Column ml;
                ml.save(outw, lane);
                const int r = bits_rescue ? tetra_list::rescue_hard<true>(p.type345, p.type2, p.a, max_candidates, ld_bits, io, half)
                                          : tetra_list::rescue_hard<false>(p.type345, p.type2, p.a, max_candidates, ld_cls, io, half);
                rank[blk] = r;
                if (r > 0) {
                    good = true;
                    if (biterr) biterr[blk] = bit_errors_hard<false>(p.type345, p.type2, p.a, half, ld_cls);
                } else {
                    ml.restore(outw, lane);
                }
            }
            crc_ok[blk] = good;
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
            auto half = [&](int h) { return outw[h][lane]; };
            bool good = decode_hard<true>(p.type345, p.type2, p.a, ld, io);
            if (biterr) biterr[blk] = bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld);
            rank[blk] = 0;
            if (!good) {
                Column ml;
                ml.save(outw, lane);
                const int r = tetra_list::rescue_hard<true>(p.type345, p.type2, p.a, max_candidates, ld, io, half);
                rank[blk] = r;
                if (r > 0) {
                    good = true;
                    if (biterr) biterr[blk] = bit_errors_hard<true>(p.type345, p.type2, p.a, half, ld);
                } else {
                    ml.restore(outw, lane);
                }
            }
            crc_ok[blk] = good;
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
            auto half = [&](int h) { return outw[h][lane]; };
            bool good = decode_soft(p.type345, p.type2, p.a, ld, io);
            if (biterr) biterr[j] = bit_errors_soft(p.type345, p.type2, p.a, half, ld);
            rank[j] = 0;
            if (!good) {
                Column ml;
                ml.save(outw, lane);
                const int r = tetra_list::rescue_soft(p.type345, p.type2, p.a, max_candidates, ld, io, half);
                rank[j] = r;
                if (r > 0) {
                    good = true;
                    if (biterr) biterr[j] = bit_errors_soft(p.type345, p.type2, p.a, half, ld);
                } else {
                    ml.restore(outw, lane);
                }
            }
            crc_ok[j] = good;
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}
