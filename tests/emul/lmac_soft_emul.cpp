// Host build of the soft-decision option's lane-level code (sdrpp-tetra-demodulator_amd/csrc/soft_core.hpp + the sequence, traceback
// and write-back of lmac_core.hpp): the quantiser of k_soft and the workgroups of k_lmac_frames_soft -- soft_core.hpp's soft_block, the
// front end the kernel calls, with lmac_lane_io.hpp's lane epilogue behind it and plain arrays where the kernels have global memory and
// LDS.  Test infrastructure: lets the CPU suite hold the exact kernel source against the reference's conv_cch_decode.
#define TETRA_HOST_EMUL 1
#include "../../sdrpp-tetra-demodulator_amd/csrc/soft_core.hpp"
#include "lmac_lane_io.hpp"

using namespace tetra_soft;
using namespace lane_emul;

extern "C" int soft_emul_q(void) { return kQ; }
extern "C" float soft_emul_g(void) { return kG; }
extern "C" float soft_emul_fresh_prev(void) { return kFreshPrev; }
extern "C" uint32_t soft_emul_ring_size(int bits_stride) { return ring_size(bits_stride); }

// k_soft for one channel: n symbols (re, im) after `prev` (in / out) -> 2 n soft values
extern "C" void soft_emul_quantise(const float* sym, int n, float* prev, int8_t* out) {
    float pr = prev[0], pi = prev[1];
    for (int k = 0; k < n; ++k) {
        int q0, q1;
        soft_pair(sym[2 * k], sym[2 * k + 1], pr, pi, q0, q1);
        out[2 * k] = (int8_t)q0;
        out[2 * k + 1] = (int8_t)q1;
        pr = sym[2 * k];
        pi = sym[2 * k + 1];
    }
    prev[0] = pr;
    prev[1] = pi;
}

// k_lmac_frames_soft, a lane per row and a 64-row workgroup at a time: row j's frame starts at absolute bit bitnum[j] of ring j (rings
// [n_rows][ring_size] int8, 4-byte aligned, ring_size a power of two), has burst type frame_type[j] and is descrambled with scramb[j]
// (NULL: SCRAMB_INIT).  out rows: type-2 bits, one per byte.
extern "C" int soft_emul_decode(int tpsap, int blk_num, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type,
                                int n_rows, const uint32_t* scramb, uint8_t* out, int out_stride, int32_t* crc_ok) {
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
            finish_lane(outw, lane, [&](LaneIo& io) { return decode_soft(p.type345, p.type2, p.a, [&](int w) { return soft[w]; }, io); },
                        [](bool) { return 0u; }, NoRescue(), &crc_ok[j], nullptr, nullptr);
        }
        write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}
