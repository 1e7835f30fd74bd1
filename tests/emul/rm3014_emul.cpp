// Host build of the AACH's Reed-Muller lane code (sdrpp-tetra-demodulator_amd/csrc/lmac_core.hpp: rm3014_encode, rm3014_syndrome,
// rm3014_correction_table, rm3014_decode) -- the source the kernels compile, with a plain array behind the table accessor.  Test
// infrastructure: tests/test_aach_rm.py checks it exhaustively without a GPU and holds the GPU entry points to it word for word.
#define TETRA_HOST_EMUL 1
#include <cstdint>
#include <vector>

#include "../../sdrpp-tetra-demodulator_amd/csrc/lmac_core.hpp"

using namespace tetra_lmac;

namespace {
const uint32_t* table() {
    static std::vector<uint32_t> tab;
    if (tab.empty()) {
        tab.resize(kRm3014TableEntries);
        rm3014_correction_table(tab.data());
    }
    return tab.data();
}
}  // namespace

extern "C" void rm3014_emul_encode(const uint32_t* info, int n, uint32_t* words) {
    for (int i = 0; i < n; ++i) words[i] = rm3014_encode(info[i]);
}

extern "C" void rm3014_emul_syndrome(const uint32_t* words, int n, uint32_t* syn) {
    for (int i = 0; i < n; ++i) syn[i] = rm3014_syndrome(words[i]);
}

extern "C" void rm3014_emul_decode(const uint32_t* words, int n, uint32_t* out_words, uint8_t* dist) {
    const uint32_t* tab = table();
    for (int i = 0; i < n; ++i) {
        const Rm3014Word r = rm3014_decode(words[i], [&](uint32_t s) { return tab[s]; });
        out_words[i] = r.word;
        dist[i] = (uint8_t)r.dist;
    }
}

// the correction table itself: entries [65536]; returns how many syndromes have a pattern
extern "C" int rm3014_emul_table(uint32_t* out) {
    const uint32_t* tab = table();
    int have = 0;
    for (uint32_t s = 0; s < kRm3014TableEntries; ++s) {
        out[s] = tab[s];
        have += tab[s] != kRm3014NoPattern;
    }
    return have;
}
