// Stand-alone sanitizer driver for the host build of the soft-decision data channels' lane code (tests/emul/lmac_tch_soft_emul.cpp,
// csrc/tch_soft_core.hpp): both coded kinds on exact-size heap buffers -- int8 byte rows at a ragged workgroup (70 rows), tight and padded
// rows, with and without counts; frames from rings that wrap (the smallest ring that holds a burst, bit numbers up to the 2^32 wrap), one
// of them of another burst type.  Built and run by tests/test_lmac_tch_soft.py with -fsanitize=address,undefined; prints
// "san_tch_soft: ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int tch_soft_emul_rows(int kind, const int8_t* soft5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                                  uint32_t* biterr);
extern "C" int tch_soft_emul_frames(int kind, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type, int n_rows,
                                    const uint32_t* scramb, uint8_t* out, int out_stride, uint32_t* biterr);

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static int8_t soft(uint32_t& s) { return (int8_t)((int)(rnd(s) % 63u) - 31); }

int main() {
    uint32_t seed = 11;
    const int type2[2] = { 292, 148 };
    for (int kind = 9; kind <= 10; ++kind) {
        const int n2 = type2[kind - 9], n = 70;
        for (int stride : { 432, 436, 448 }) {
            std::vector<int8_t> rows((size_t)n * stride);
            std::vector<uint8_t> out((size_t)n * n2), out2((size_t)n * n2);
            std::vector<uint32_t> code(n), be(n);
            for (auto& v : rows) v = soft(seed);
            for (auto& c : code) c = rnd(seed) * 977u;
            if (tch_soft_emul_rows(kind, rows.data(), n, stride, code.data(), out.data(), n2, be.data())) return 1;
            if (tch_soft_emul_rows(kind, rows.data(), n, stride, code.data(), out2.data(), n2, nullptr)) return 2;
            if (std::memcmp(out.data(), out2.data(), out.size())) return 3;                  // counting changes no bit
            for (int j = 0; j < n; ++j)
                if ((be[j] >> 16) > 432u || (be[j] & 0xffffu) > (be[j] >> 16)) return 4;
        }
        // rings of 512 values: every frame wraps somewhere; the row's values are in the ring already (junk is as good as a row here)
        const int nf = 67, ost = (n2 + 7) & ~7;
        const uint32_t ring_size = 512;
        std::vector<int8_t> rings((size_t)nf * ring_size);
        std::vector<uint32_t> bitnum(nf), scramb(nf), be(nf);
        std::vector<int32_t> ftype(nf);
        for (auto& v : rings) v = soft(seed);
        for (int f = 0; f < nf; ++f) {
            bitnum[f] = f < 8 ? (uint32_t)f : f < 16 ? 0xffffffffu - (uint32_t)(37 * f) : rnd(seed) * 2654435761u;
            scramb[f] = rnd(seed) * 977u;
            ftype[f] = f % 9 == 4 ? 3 : f % 9 == 7 ? 1 : 0;            // a SYNC and a NORM_2 burst now and then: erasures
        }
        std::vector<uint8_t> out((size_t)nf * ost), out2((size_t)nf * ost);
        if (tch_soft_emul_frames(kind, rings.data(), ring_size, bitnum.data(), ftype.data(), nf, scramb.data(), out.data(), ost, be.data())) return 5;
        if (tch_soft_emul_frames(kind, rings.data(), ring_size, bitnum.data(), ftype.data(), nf, scramb.data(), out2.data(), ost, nullptr)) return 6;
        if (std::memcmp(out.data(), out2.data(), out.size())) return 7;
        for (int f = 0; f < nf; ++f)
            if (ftype[f] != 0 && be[f] != 0u) return 8;               // a frame of another burst type compares nothing
    }
    std::printf("san_tch_soft: ok\n");
    return 0;
}
