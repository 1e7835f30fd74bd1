// Host build of the soft-decision option's lane-level code (sdrpp-tetra-demodulator_amd/csrc/soft_core.hpp + the traceback of
// lmac_core.hpp): the quantiser of k_soft and one lane of k_lmac_frames_soft with plain arrays where the kernels have global memory
// and LDS.  Test infrastructure: lets the CPU suite hold the exact kernel source against the reference's conv_cch_decode.
#define TETRA_HOST_EMUL 1
#include <cstdint>
#include <cstring>

#include "../../sdrpp-tetra-demodulator_amd/csrc/soft_core.hpp"

using namespace tetra_soft;

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

// One lane of k_lmac_frames_soft per row: row j's frame starts at absolute bit bitnum[j] of ring j (rings [n_rows][ring_size] int8,
// 4-byte aligned, ring_size a power of two), has burst type frame_type[j] and is descrambled with scramb[j] (NULL: SCRAMB_INIT).
// out rows: type-2 bits, one per byte.
extern "C" int soft_emul_decode(int tpsap, int blk_num, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type,
                                int n_rows, const uint32_t* scramb, uint8_t* out, int out_stride, int32_t* crc_ok) {
    int layout = kLayoutNone, type345 = 0, type2 = 0, a = 0;
    switch (tpsap) {
        case TETRA_TPSAP_T_SB1: layout = blk_num == 1 ? kLayoutSb1 : kLayoutNone; type345 = 120; type2 = 80; a = 11; break;
        case TETRA_TPSAP_T_SB2: layout = blk_num == 2 ? kLayoutSb2 : kLayoutNone; type345 = 216; type2 = 144; a = 101; break;
        case TETRA_TPSAP_T_NDB: layout = blk_num == 1 ? kLayoutNdb1 : blk_num == 2 ? kLayoutNdb2 : kLayoutNone; type345 = 216; type2 = 144; a = 101; break;
        case TETRA_TPSAP_T_SCH_F: layout = kLayoutSchF; type345 = 432; type2 = 288; a = 103; break;
        default: break;
    }
    if (layout == kLayoutNone || ring_size < 4 || (ring_size & (ring_size - 1))) return -1;
    static const CrcInvTable crci = make_crc_inv_table();
    for (int j = 0; j < n_rows; ++j) {
        const uint32_t* ring = reinterpret_cast<const uint32_t*>(rings + (size_t)j * ring_size);
        uint32_t seq[kSeqWords], soft[kSoftWords] = {}, dec[(kMaxType2 + kFlush) / 2];
        uint16_t outw[kMaxType2 / 16];
        scramb_sequence_words(scramb ? scramb[j] : kScrambInitSb1, seq);
        stage_block(layout, bitnum[j], frame_type[j], [&](uint32_t w) { return ring[w]; }, ring_size - 1u, seq, [&](int g, uint32_t word) { soft[g] = word; });
        forward(type345, type2, a, [&](int w) { return soft[w]; }, [&](int u, uint32_t word) { dec[u] = word; });
        crc_ok[j] = viterbi_traceback(type2, [&](int u) { return dec[u]; }, [&](int h, uint32_t half) { outw[h] = (uint16_t)half; },
                                      [&](uint32_t off) { return crci.t[off >> 2]; });
        for (int t4 = 0; t4 < type2 / 4; ++t4) {
            const uint32_t v = spread4((outw[t4 >> 2] >> (4 * (t4 & 3))) & 0xfu);
            std::memcpy(out + (size_t)j * out_stride + 4 * t4, &v, 4);
        }
    }
    return 0;
}
