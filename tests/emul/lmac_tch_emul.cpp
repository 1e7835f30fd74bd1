// Host build of the circuit-mode data channels' lane code (include/ext/tetra_tch.h; csrc/tch_core.hpp) behind the decoder's front ends
// -- what k_tch_rows and k_tch_frames run.  Each entry is a loop over workgroups and lanes that picks the front end the kernel calls
// (lmac_core.hpp; the cooperative stage of byte rows is lmac_lane_io.hpp's stage_workgroup) and runs tch_core.hpp's decode_lane behind it.
// Test infrastructure: lets the CPU suite hold the exact lane source against the reference's primitives without a GPU.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/tch_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_tch;
using lane_emul::frame_rows;
using lane_emul::row_words;
using lane_emul::seq_rows;
using lane_emul::seq_table;
using lane_emul::stage_workgroup;

namespace {

typedef uint16_t TchOutW[kOutHalves][kLanes];
struct TchIo {
    TchOutW& outw;
    int lane;
    uint32_t dec[kMaxPairs];
    void dec_st(int u, uint32_t w) { dec[u] = w; }
    uint32_t dec_ld(int u) const { return dec[u]; }
    void out_st(int h, uint32_t half) { outw[h][lane] = (uint16_t)half; }
    uint32_t out_ld(int h) const { return outw[h][lane]; }
};

void write_out(const TchOutW& outw, int rows_here, int type2, uint8_t* out0, int out_stride) {
    for (int lane = 0; lane < kLanes; ++lane)
        tetra_tch::write_rows(lane, rows_here, type2, rows_wide(out0, out_stride), [&](int h, int q) { return outw[h][q]; },
                              [&](int q, int d, demux_core::U2 v) { std::memcpy(out0 + (size_t)q * out_stride + 8 * d, &v, 8); },
                              [&](int q, int d, uint32_t v) { std::memcpy(out0 + (size_t)q * out_stride + 4 * d, &v, 4); });
}

}  // namespace

// k_tch_rows.  route: 0 = like the kernel (a workgroup of plain-bit rows, 8-byte aligned and at most 512 bytes apart, takes the packed
// route, any other the byte route), 1 = byte route always.  biterr [n_blocks] may be NULL; fast_rows: the rows of the workgroups that
// took the packed route.
extern "C" int tch_emul_rows(int kind, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                             uint32_t* biterr, int route, int32_t* fast_rows) {
    if (!is_tch(kind) || (in_stride & 3) || (out_stride & 3)) return -1;
    const Kind k = kind_of(kind);
    const BlockKind bk{ kLayoutNone, kType345 };
    const uint32_t* seq_tab = route == 0 ? seq_table() : nullptr;
    int fast = 0;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        const uint8_t* rows = type5 + (size_t)blk0 * in_stride;
        uint8_t* out0 = out + (size_t)blk0 * out_stride;
        if (k.ng == 0) {
            uint32_t seq[kLanes][kSeqWords] = {};
            for (int lane = 0; lane < rows_here; ++lane)
                lane_sequence(kType345, scramb_init[blk0 + lane], seq_rows(seq_table()), [&](int w, uint32_t word) { seq[lane][w] = word; });
            for (int lane = 0; lane < kLanes; ++lane)
                passthrough_rows(lane, rows_here, [&](int w, int q) { return seq[q][w]; },
                                 [&](int q, int d) { uint32_t v; std::memcpy(&v, rows + (size_t)q * in_stride + 4 * d, 4); return v; },
                                 [&](int q, int d, uint32_t v) { std::memcpy(out0 + (size_t)q * out_stride + 4 * d, &v, 4); });
            continue;
        }
        uint32_t xb[kLanes][kSeqWords];
        const bool packed = stage_workgroup(seq_tab, kType345, type5, rows, rows_here, in_stride, xb);
        if (packed) fast += rows_here;
        TchOutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            uint32_t cls[kClsWords + 1];
            auto ld = [&](int w) { return cls[w]; };
            auto st = [&](int w, uint32_t word) { cls[w] = word; };
            TchIo io{ outw, lane, {} };
            uint32_t be;
            if (packed) {
                descramble_words(kType345, scramb_init[blk], xb[lane], seq_rows(seq_tab), st);
                be = decode_lane<true>(k.ng, k.type2, biterr != nullptr, ld, io);
            } else {
                byte_row_block(&bk, scramb_init[blk], row_words(rows + (size_t)lane * in_stride), st);
                be = decode_lane<false>(k.ng, k.type2, biterr != nullptr, ld, io);
            }
            if (biterr) biterr[blk] = be;
        }
        write_out(outw, rows_here, k.type2, out0, out_stride);
    }
    if (fast_rows) *fast_rows = fast;
    return 0;
}

// k_tch_frames, one job: the listed frames (frames [n_frames][16] packed, frame_scramb per frame slot); biterr may be NULL
extern "C" int tch_emul_frames(int kind, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame, int n_rows,
                               const uint32_t* frame_scramb, uint8_t* out, int out_stride, uint32_t* biterr) {
    if (!is_tch(kind) || (out_stride & 3)) return -1;
    const Kind k = kind_of(kind);
    const BlockKind bk{ kLayoutSchF, kType345 };
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        uint8_t* out0 = out + (size_t)blk0 * out_stride;
        TchOutW outw;
        uint32_t bits[kLanes][kSeqWords] = {};
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            const FrameRef fr = lane_emul::frame_of(TETRA_TPSAP_T_SCH_F, row_frame, blk, frame_scramb);
            uint32_t fw[kFrameWords];
            load_frame(frame_rows(frames, fr.f), fw);
            frame_hard_block(&bk, fr.code, fw, [&] { return frame_type[fr.f]; }, seq_rows(seq_table()), [&](int w, uint32_t word) { bits[lane][w] = word; });
            if (k.ng == 0) continue;
            TchIo io{ outw, lane, {} };
            const uint32_t be = decode_lane<true>(k.ng, k.type2, biterr != nullptr, [&](int w) { return bits[lane][w]; }, io);
            if (biterr) biterr[blk] = be;
        }
        if (k.ng == 0) {
            for (int lane = 0; lane < kLanes; ++lane)
                passthrough_rows(lane, rows_here, [&](int w, int q) { return bits[q][w]; }, [&](int, int) { return 0u; },
                                 [&](int q, int d, uint32_t v) { std::memcpy(out0 + (size_t)q * out_stride + 4 * d, &v, 4); });
        } else {
            write_out(outw, rows_here, k.type2, out0, out_stride);
        }
    }
    return 0;
}

// the schedule as the kernels know it: pattern[u] = pair_pattern of step pair u, for the n2 / 2 pairs of the kind
extern "C" int tch_emul_schedule(int kind, uint8_t* pattern) {
    if (!is_tch(kind) || kind_of(kind).ng == 0) return -1;
    const Kind k = kind_of(kind);
    for (int u = 0; u < k.type2 / 2; ++u) pattern[u] = (uint8_t)pair_pattern(k.ng, u);
    return k.type2 / 2;
}
