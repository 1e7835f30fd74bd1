// Host build of the soft-decision data channels' lane code (include/ext/tetra_tch_soft.h; csrc/tch_soft_core.hpp) behind its two front
// ends -- what k_tch_rows_soft and k_tch_frames_soft run.  Each entry is a loop over workgroups and lanes with plain arrays where the
// kernels have LDS and global memory.  Test infrastructure: lets the CPU suite hold the exact lane source against the reference's
// conv_cch_decode behind its TCH puncturers without a GPU.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/tch_soft_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_tch_soft;
using lane_emul::ring_words;
using lane_emul::row_words;
using lane_emul::seq_rows;
using lane_emul::seq_table;

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

// a workgroup behind its front end: stage(lane, soft) fills the lane's staged block
template <class Stage>
void workgroup(const Kind& k, int blk0, int rows_here, Stage stage, uint8_t* out0, int out_stride, uint32_t* biterr) {
    TchOutW outw;
    for (int lane = 0; lane < rows_here; ++lane) {
        uint32_t soft[kSoftWords] = {};
        stage(lane, soft);
        TchIo io{ outw, lane, {} };
        const uint32_t be = decode_lane(k.ng, k.type2, biterr != nullptr, [&](int w) { return soft[w]; }, io);
        if (biterr) biterr[blk0 + lane] = be;
    }
    write_out(outw, rows_here, k.type2, out0, out_stride);
}

}  // namespace

// k_tch_rows_soft: int8 rows [n_blocks][in_stride]; biterr [n_blocks] may be NULL
extern "C" int tch_soft_emul_rows(int kind, const int8_t* soft5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                                  uint32_t* biterr) {
    if (!is_tch(kind) || kind_of(kind).ng == 0 || (in_stride & 3) || (out_stride & 3)) return -1;
    const Kind k = kind_of(kind);
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        workgroup(k, blk0, rows_here, [&](int lane, uint32_t* soft) {
            const uint8_t* row = reinterpret_cast<const uint8_t*>(soft5) + (size_t)(blk0 + lane) * in_stride;
            stage_row(scramb_init[blk0 + lane], seq_rows(seq_table()), row_words(row), [&](int g, uint32_t word) { soft[g] = word; });
        }, out + (size_t)blk0 * out_stride, out_stride, biterr);
    }
    return 0;
}

// k_tch_frames_soft, one job: row j's frame starts at absolute bit bitnum[j] of ring j (rings [n_rows][ring_size] int8, 4-byte aligned,
// ring_size a power of two), has burst type frame_type[j] and scrambling code scramb[j]; biterr may be NULL
extern "C" int tch_soft_emul_frames(int kind, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type, int n_rows,
                                    const uint32_t* scramb, uint8_t* out, int out_stride, uint32_t* biterr) {
    if (!is_tch(kind) || kind_of(kind).ng == 0 || (out_stride & 3) || ring_size < 4 || (ring_size & (ring_size - 1))) return -1;
    const Kind k = kind_of(kind);
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        workgroup(k, blk0, rows_here, [&](int lane, uint32_t* soft) {
            const int j = blk0 + lane;
            frame_block(scramb[j], [&] { return bitnum[j]; }, [&] { return frame_type[j]; }, seq_rows(seq_table()),
                        ring_words(rings + (size_t)j * ring_size), ring_size / 4u, [&](int g, uint32_t word) { soft[g] = word; });
        }, out + (size_t)blk0 * out_stride, out_stride, biterr);
    }
    return 0;
}
