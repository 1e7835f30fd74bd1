// What the host emulations of the lower-MAC decoder (lmac_emul.cpp, lmac_soft_emul.cpp) put behind the lane code's accessors where the
// kernels have LDS and the global decision scratch: a workgroup is a loop over 64 lanes, its shared arrays are plain arrays.
#pragma once
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

}  // namespace lane_emul
