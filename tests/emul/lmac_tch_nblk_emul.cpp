// Host build of the N-block front end of the coded data channels (include/ext/tetra_tch_nblk.h; csrc/tch_nblk_core.hpp) in front of the
// lane code it hands to (tch_core.hpp, tch_soft_core.hpp) -- what k_tch_nblk and k_tch_nblk_soft run.  Each entry is a loop over
// workgroups and lanes with plain arrays where the kernels have LDS and global memory.  Test infrastructure: lets the CPU suite hold the
// exact lane source against the clause and the reference's functions (tests/tch_nblk_definition.py) without a GPU.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/tch_nblk_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_tch_nblk;
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

bool args_ok(int kind, int n, int in_stride, int out_stride) {
    return is_tch(kind) && kind_of(kind).ng != 0 && valid_n(n) && !(in_stride & 3) && !(out_stride & 3);
}

}  // namespace

// k_tch_nblk.  pool uint8 [n_rows][in_stride], the code of pool row r is scramb_init[init_index ? init_index[r] : r]; windows
// [n_blocks][n].  route: 0 = like the kernel (a workgroup of complete windows over plain-bit rows takes the packed route, any other the
// class route), 1 = class route always.  biterr [n_blocks] may be NULL; fast_blocks: the blocks of the workgroups that took the packed route.
extern "C" int tch_nblk_emul_hard(int kind, int n, const uint8_t* pool, int n_rows, int in_stride, const uint32_t* scramb_init, const int32_t* init_index,
                                  const int32_t* windows, int n_blocks, uint8_t* out, int out_stride, uint32_t* biterr, int route, int32_t* fast_blocks) {
    if (!args_ok(kind, n, in_stride, out_stride)) return -1;
    const Kind k = kind_of(kind);
    int fast = 0;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        uint32_t cls[kLanes][kClsWords + 1] = {};
        uint32_t dirty = 0;                                           // the kernel's ballot
        for (int lane = 0; lane < rows_here; ++lane) {
            uint32_t seq[kSeqWords];
            const int32_t* win = windows + (size_t)(blk0 + lane) * n;
            dirty |= gather_hard(n, n_rows, [&](int j) { return win[j]; }, [&](int r) { return scramb_init[init_index ? init_index[r] : r]; },
                                 seq_rows(seq_table()), [&](int w, uint32_t word) { seq[w] = word; }, [&](int w) { return seq[w]; },
                                 [&](int r, int t) -> uint32_t { return pool[(size_t)r * in_stride + t]; },
                                 [&](int w, uint32_t bits) { cls[lane][w] |= bits; });
        }
        const bool class_route = route != 0 || dirty != 0;
        if (!class_route) fast += rows_here;
        TchOutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            auto ld = [&](int w) { return cls[lane][w]; };
            TchIo io{ outw, lane, {} };
            uint32_t be;
            if (!class_route) {
                classes_to_bits(ld, [&](int w, uint32_t word) { cls[lane][w] = word; });
                be = tetra_tch::decode_lane<true>(k.ng, k.type2, biterr != nullptr, ld, io);
            } else {
                be = tetra_tch::decode_lane<false>(k.ng, k.type2, biterr != nullptr, ld, io);
            }
            if (biterr) biterr[blk0 + lane] = be;
        }
        write_out(outw, rows_here, k.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    if (fast_blocks) *fast_blocks = fast;
    return 0;
}

// k_tch_nblk_soft: pool int8 [n_rows][in_stride]; everything else as above
extern "C" int tch_nblk_emul_soft(int kind, int n, const int8_t* pool, int n_rows, int in_stride, const uint32_t* scramb_init, const int32_t* init_index,
                                  const int32_t* windows, int n_blocks, uint8_t* out, int out_stride, uint32_t* biterr) {
    if (!args_ok(kind, n, in_stride, out_stride)) return -1;
    const Kind k = kind_of(kind);
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(pool);
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        TchOutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            uint32_t seq[kSeqWords], soft[kSoftWords];
            for (int g = 0; g < kSoftWords; ++g) soft[g] = 0x80808080u;
            const int32_t* win = windows + (size_t)(blk0 + lane) * n;
            gather_soft(n, n_rows, [&](int j) { return win[j]; }, [&](int r) { return scramb_init[init_index ? init_index[r] : r]; },
                        seq_rows(seq_table()), [&](int w, uint32_t word) { seq[w] = word; }, [&](int w) { return seq[w]; },
                        [&](int r, int t) -> uint32_t { return bytes[(size_t)r * in_stride + t]; },
                        [&](int q, uint32_t y) { soft[q >> 2] = (soft[q >> 2] & ~(0xffu << (8 * (q & 3)))) | (y << (8 * (q & 3))); });
            TchIo io{ outw, lane, {} };
            const uint32_t be = decode_lane(k.ng, k.type2, biterr != nullptr, [&](int w) { return soft[w]; }, io);
            if (biterr) biterr[blk0 + lane] = be;
        }
        write_out(outw, rows_here, k.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}
