// Stand-alone sanitizer run of the burst synchroniser's tolerant lock (host build of csrc/bsync_core.hpp, tests/emul/bsync_tol_emul.cpp):
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o san_sync_tol san_sync_tol.cpp && ./san_sync_tol streams.bin
// streams.bin: per stream an int32 bit count and that many bytes, one per bit (tests/test_sync_tol.py writes the adversarial streams).
// Every stream runs under every parameter set, cut into calls of every size the CPU tests use, with exactly-sized heap buffers so that a
// read or write past an end is seen; the three ways of walking the LOCKED frames must report the same.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../emul/bsync_tol_emul.cpp"

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    const int32_t params[4][3] = { { 0, 0, 1 }, { 3, 5, 16 }, { 4, 6, 255 }, { 2, 2, 2 } };
    const int cuts[] = { 1, 509, 510, 511, 1019, 4096, 33661, 0 };
    long long frames_total = 0, reported_total = 0;
    uint64_t sum = 1469598103934665603ull;
    int32_t n = 0, n_streams = 0;
    while (std::fread(&n, sizeof(n), 1, f) == 1) {
        if (n < 0 || n > (1 << 24)) { std::fprintf(stderr, "bad stream length %d\n", n); return 2; }
        std::vector<uint8_t> bits((size_t)n);
        if (n && std::fread(bits.data(), 1, (size_t)n, f) != (size_t)n) { std::fprintf(stderr, "short stream\n"); return 2; }
        n_streams++;
        for (const auto& tol : params)
            for (int cut : cuts) {
                if (cut == 1 && n > 6000) continue;                 // (one bit per call: the short streams)
                uint64_t per_mode[3] = { 0, 0, 0 };
                for (int mode = 0; mode < 3; ++mode) {
                    State st = {};
                    int32_t misses = 0;
                    std::vector<uint8_t> carry(4096, 0);
                    uint64_t h = 1469598103934665603ull;
                    int pos = 0, empty_done = 0;
                    while (pos < n || !empty_done) {
                        const int len = cut == 0 ? (empty_done ? n - pos : 0) : (n - pos < cut ? n - pos : cut);
                        empty_done = 1;
                        const int cap = (4096 + len) / 510 + 2;
                        std::vector<uint8_t> chunk(bits.begin() + pos, bits.begin() + pos + len), fr((size_t)cap * 512);
                        std::vector<int32_t> ty((size_t)cap);
                        std::vector<uint32_t> bn((size_t)cap);
                        const int got = bsync_tol_emul_process(&st, &misses, carry.data(), chunk.data(), len, tol, fr.data(), ty.data(), bn.data(), cap, mode);
                        if (got < 0) { std::fprintf(stderr, "process failed: %d\n", got); return 1; }
                        for (int k = 0; k < got; ++k) {
                            h = (h ^ (uint64_t)(uint32_t)ty[k]) * 1099511628211ull;
                            h = (h ^ bn[k]) * 1099511628211ull;
                            for (int i = 0; i < 510; i += 51) h = (h ^ fr[(size_t)k * 512 + i]) * 1099511628211ull;
                            if (mode == 0) { frames_total++; reported_total += ty[k] >= 0; }
                        }
                        pos += len;
                    }
                    h = (h ^ (uint64_t)st.state ^ ((uint64_t)st.bits_in_buf << 8) ^ ((uint64_t)st.bitbuf_start_bitnum << 24) ^ ((uint64_t)(uint32_t)misses << 48)) * 1099511628211ull;
                    per_mode[mode] = h;
                }
                if (per_mode[0] != per_mode[1] || per_mode[0] != per_mode[2]) { std::fprintf(stderr, "the walks disagree (stream %d, cut %d)\n", n_streams, cut); return 1; }
                sum = (sum ^ per_mode[0]) * 1099511628211ull;
            }
    }
    std::fclose(f);
    if (n_streams == 0 || reported_total == 0) { std::fprintf(stderr, "nothing ran\n"); return 1; }
    std::printf("san_sync_tol ok: streams=%d frames=%lld reported=%lld checksum=%016llx\n", n_streams, frames_total, reported_total, (unsigned long long)sum);
    return 0;
}
