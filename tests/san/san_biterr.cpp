// AddressSanitizer / UBSan driver for the host build of the channel bit-error count (tests/emul/lmac_biterr_emul.cpp: reencode_errors of
// csrc/lmac_core.hpp behind the decoder's three front ends), on exact-size heap buffers: a read or write past a row, a staged block or a
// count array is a report, and a report is a non-zero exit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int biterr_emul_rows(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                                int32_t* crc_ok, uint32_t* biterr, int route, int32_t* fast_rows);
extern "C" int biterr_emul_frames(int tpsap, int blk_num, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame, int n_rows,
                                  const uint32_t* frame_scramb, uint8_t* out, int out_stride, int32_t* crc_ok, uint32_t* biterr);
extern "C" int biterr_emul_soft(int tpsap, int blk_num, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type,
                                int n_rows, const uint32_t* scramb, uint8_t* out, int out_stride, int32_t* crc_ok, uint32_t* biterr);

static uint32_t rnd_state = 12345u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "san_biterr: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

int main() {
    static const int kinds[5][3] = { { 0, 120, 80 }, { 1, 216, 144 }, { 2, 216, 144 }, { 4, 168, 112 }, { 5, 432, 288 } };      // type, type345, type2
    for (const auto& k : kinds) {
        const int n = 70;                                    // a full workgroup and a ragged one
        for (int stride : { k[1], (k[1] + 7) / 8 * 8 + 8 }) {
            std::vector<uint8_t> rows((size_t)n * stride), out((size_t)n * k[2]);
            for (auto& b : rows) b = (uint8_t)(rnd() >> 31);
            rows[(size_t)66 * stride + 3] = 0xff;            // the second workgroup takes the byte route
            std::vector<uint32_t> code(n), be(n);
            for (auto& c : code) c = rnd();
            std::vector<int32_t> ok(n);
            for (int route = 0; route < 2; ++route) {
                int32_t fast = -1;
                REQUIRE(biterr_emul_rows(k[0], rows.data(), n, stride, code.data(), out.data(), k[2], ok.data(), be.data(), route, &fast) == 0);
                for (int j = 0; j < n; ++j) REQUIRE((be[j] >> 16) <= (uint32_t)k[1] && (be[j] & 0xffffu) <= (be[j] >> 16));
            }
        }
    }
    {
        const int nf = 24;
        std::vector<uint32_t> frames((size_t)nf * 16), code(nf);
        std::vector<int32_t> ft(nf), list(nf);
        for (auto& w : frames) w = rnd();
        for (int f = 0; f < nf; ++f) { code[f] = rnd(); ft[f] = (int)(rnd() >> 30); list[f] = nf - 1 - f; }
        static const int jobs[5][3] = { { 0, 1, 80 }, { 1, 2, 144 }, { 2, 1, 144 }, { 2, 2, 144 }, { 5, 0, 288 } };
        for (const auto& j : jobs) {
            std::vector<uint8_t> out((size_t)nf * j[2]);
            std::vector<int32_t> ok(nf);
            std::vector<uint32_t> be(nf);
            REQUIRE(biterr_emul_frames(j[0], j[1], frames.data(), ft.data(), list.data(), nf, code.data(), out.data(), j[2], ok.data(), be.data()) == 0);
            const uint32_t ring = 1024;
            std::vector<int8_t> rings((size_t)nf * ring);
            for (auto& v : rings) v = (int8_t)((int)(rnd() >> 26) - 32 < -31 ? 0 : (int)(rnd() >> 26) - 32);
            std::vector<uint32_t> bn(nf);
            for (auto& b : bn) b = rnd();
            REQUIRE(biterr_emul_soft(j[0], j[1], rings.data(), ring, bn.data(), ft.data(), nf, code.data(), out.data(), j[2], ok.data(), be.data()) == 0);
        }
    }
    std::puts("san_biterr: ok");
    return 0;
}
