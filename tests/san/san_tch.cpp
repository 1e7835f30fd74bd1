// Stand-alone sanitizer driver for the host build of the circuit-mode data channels' lane code (tests/emul/lmac_tch_emul.cpp,
// csrc/tch_core.hpp): every kind on exact-size heap buffers -- byte rows at a ragged workgroup (70 rows) through both routes, tight
// and padded rows, with and without counts; frames of every burst type.  Built and run by tests/test_lmac_tch.py with
// -fsanitize=address,undefined; prints "san_tch: ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int tch_emul_rows(int kind, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init, uint8_t* out, int out_stride,
                             uint32_t* biterr, int route, int32_t* fast_rows);
extern "C" int tch_emul_frames(int kind, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame, int n_rows,
                               const uint32_t* frame_scramb, uint8_t* out, int out_stride, uint32_t* biterr);
extern "C" int tch_emul_schedule(int kind, uint8_t* pattern);

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    uint32_t seed = 7;
    const int type2[3] = { 432, 292, 148 };
    for (int kind = 8; kind <= 10; ++kind) {
        const int n2 = type2[kind - 8], n = 70;
        for (int stride : { 432, 436, 440 }) {
            for (int dirty = 0; dirty < 2; ++dirty) {
                std::vector<uint8_t> rows((size_t)n * stride), out((size_t)n * n2), out2((size_t)n * n2);
                std::vector<uint32_t> code(n), be(n), be2(n);
                for (auto& b : rows) b = dirty ? (uint8_t)rnd(seed) : (uint8_t)(rnd(seed) & 1u);
                for (auto& c : code) c = rnd(seed) * 977u;
                int32_t fast = -1;
                const bool coded = kind != 8;
                if (tch_emul_rows(kind, rows.data(), n, stride, code.data(), out.data(), n2, coded ? be.data() : nullptr, 0, &fast)) return 1;
                if (tch_emul_rows(kind, rows.data(), n, stride, code.data(), out2.data(), n2, coded ? be2.data() : nullptr, 1, nullptr)) return 2;
                if (std::memcmp(out.data(), out2.data(), out.size()) || (coded && std::memcmp(be.data(), be2.data(), 4 * n))) return 3;      // both routes agree
                if (coded && fast != ((stride & 7) || dirty ? 0 : n)) return 4;
                if (tch_emul_rows(kind, rows.data(), n, stride, code.data(), out2.data(), n2, nullptr, 0, nullptr)) return 5;
                if (std::memcmp(out.data(), out2.data(), out.size())) return 6;
            }
        }
        const int nf = 9, rows_n = 9, ost = (n2 + 7) & ~7;
        std::vector<uint32_t> frames((size_t)nf * 16), scramb(nf), be(rows_n);
        std::vector<int32_t> ftype(nf), list(rows_n);
        for (auto& w : frames) w = rnd(seed) * 2654435761u;
        for (int f = 0; f < nf; ++f) { scramb[f] = rnd(seed); ftype[f] = f % 5 == 4 ? -1 : f % 5; list[f] = nf - 1 - f; }
        std::vector<uint8_t> out((size_t)rows_n * ost);
        if (tch_emul_frames(kind, frames.data(), ftype.data(), list.data(), rows_n, scramb.data(), out.data(), ost, kind != 8 ? be.data() : nullptr)) return 7;
        if (kind != 8) {
            std::vector<uint8_t> pat(n2 / 2);
            if (tch_emul_schedule(kind, pat.data()) != n2 / 2) return 8;
        }
    }
    std::printf("san_tch: ok\n");
    return 0;
}
