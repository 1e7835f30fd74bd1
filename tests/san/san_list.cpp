// AddressSanitizer / UBSan driver for the host build of the CRC-aided list decoding (tests/emul/lmac_list_emul.cpp: list_core.hpp behind
// the decoder's three front ends), on exact-size heap buffers: a read or write past a row, a staged block, a decision array or a rank
// array is a report, and a report is a non-zero exit.  Random rows fail the CRC, so every row goes through the rescue.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

extern "C" int list_emul_rows(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                              int32_t* crc_ok, int32_t* rank, uint32_t* biterr, int route, int max_candidates, int bits_rescue);
extern "C" int list_emul_frames(int tpsap, int blk_num, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame, int n_rows,
                                const uint32_t* frame_scramb, uint8_t* out, int out_stride, int32_t* crc_ok, int32_t* rank, uint32_t* biterr,
                                int max_candidates);
extern "C" int list_emul_soft(int tpsap, int blk_num, const int8_t* rings, uint32_t ring_size, const uint32_t* bitnum, const int32_t* frame_type,
                              int n_rows, const uint32_t* scramb, uint8_t* out, int out_stride, int32_t* crc_ok, int32_t* rank, uint32_t* biterr,
                              int max_candidates);

static uint32_t rnd_state = 2468u;
static uint32_t rnd() { return rnd_state = rnd_state * 1664525u + 1013904223u; }

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "san_list: %s failed at line %d\n", #c, __LINE__); return 1; } } while (0)

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
            std::vector<int32_t> ok(n), rank(n);
            for (int route = 0; route < 2; ++route)
                for (int T : { 1, 4, 8 }) {
                    REQUIRE(list_emul_rows(k[0], rows.data(), n, stride, code.data(), out.data(), k[2], ok.data(), rank.data(), T == 4 ? nullptr : be.data(), route, T, 0) == 0);
                    for (int j = 0; j < n; ++j) REQUIRE(rank[j] >= -1 && rank[j] <= T && (ok[j] != 0) == (rank[j] >= 0));
                }
            REQUIRE(list_emul_rows(k[0], rows.data(), 64, stride, code.data(), out.data(), k[2], ok.data(), rank.data(), be.data(), 0, 8, 1) == (stride % 8 ? -2 : 0));
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
            std::vector<int32_t> ok(nf), rank(nf);
            std::vector<uint32_t> be(nf);
            REQUIRE(list_emul_frames(j[0], j[1], frames.data(), ft.data(), list.data(), nf, code.data(), out.data(), j[2], ok.data(), rank.data(), be.data(), 8) == 0);
            const uint32_t ring = 1024;
            std::vector<int8_t> rings((size_t)nf * ring);
            for (auto& v : rings) v = (int8_t)((int)(rnd() >> 26) - 32 < -31 ? 0 : (int)(rnd() >> 26) - 32);
            std::vector<uint32_t> bn(nf);
            for (auto& b : bn) b = rnd();
            REQUIRE(list_emul_soft(j[0], j[1], rings.data(), ring, bn.data(), ft.data(), nf, code.data(), out.data(), j[2], ok.data(), rank.data(), be.data(), 8) == 0);
            for (int r = 0; r < nf; ++r) REQUIRE(rank[r] >= -1 && rank[r] <= 8);
        }
    }
    std::puts("san_list: ok");
    return 0;
}
