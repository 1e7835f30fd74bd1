// test_aach_soft_bank.cpp -- TetraRxBank::setAachMinMargin / fetchAachMargin and their TetraRxMultiBank pass-through (host/tetra_rx_bank.h)
// on a GPU (TEST TOOL, plain build).
//   test_aach_soft_bank <C> <N> <calls> <iq.bin> <shards> <min_margin>
// streams <calls> blocks of C x N complex64 samples (channel major, one after the other in the file) through ONE bank of C channels and
// through a bank of <shards> shards on device 0, both with TETRA_RX_FLAG_SOFT | TETRA_RX_FLAG_AACH_SOFT and the given min_margin, and
// through a bank with TETRA_RX_FLAG_SOFT alone.  After every call the shards' BBK rows and margins, one after the other, must be the
// single bank's; a row's verdict is margin >= min_margin; the soft-only bank has the same BBK rows' labels and refuses both entries.
// Prints: test_aach_soft_bank: ok rows <n> refused <n>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

static int fail(const char* what, long long v) { std::fprintf(stderr, "test_aach_soft_bank: %s (%lld)\n", what, v); return 1; }

int main(int argc, char** argv) {
    if (argc != 7) return fail("usage", argc);
    const int C = std::atoi(argv[1]), N = std::atoi(argv[2]), calls = std::atoi(argv[3]), shards = std::atoi(argv[5]), mm = std::atoi(argv[6]);
    std::vector<float> iq((size_t)2 * C * N);
    std::FILE* in = std::fopen(argv[4], "rb");
    if (!in) return fail("input file", 0);
    tetra_rx_config_t cfg;
    tetra_rx_default_config(&cfg);
    cfg.demod.n_channels = C;
    cfg.demod.max_samples = N;
    TetraRxBank plain, one, bad;
    TetraRxMultiBank many;
    cfg.flags = TETRA_RX_FLAG_AACH_SOFT;
    if (bad.init(cfg) != TETRA_ERR_ARG) return fail("the flag without TETRA_RX_FLAG_SOFT", 0);
    cfg.flags = TETRA_RX_FLAG_SOFT | TETRA_RX_FLAG_AACH_SOFT | TETRA_RX_FLAG_AACH_RM3014;
    if (bad.init(cfg) != TETRA_ERR_ARG) return fail("the flag beside TETRA_RX_FLAG_AACH_RM3014", 0);
    cfg.flags = TETRA_RX_FLAG_SOFT;
    int rc = plain.init(cfg);
    if (rc != TETRA_OK) return fail("init soft-only", rc);
    std::vector<uint16_t> none;
    if (plain.setAachMinMargin(1) != TETRA_ERR_UNSUPPORTED || plain.fetchAachMargin(none) != TETRA_ERR_UNSUPPORTED) return fail("without the flag", 0);
    cfg.flags = TETRA_RX_FLAG_SOFT | TETRA_RX_FLAG_AACH_SOFT;
    if ((rc = one.init(cfg)) != TETRA_OK) return fail("init", rc);
    if ((rc = many.init(cfg, std::vector<int>((size_t)shards, 0))) != TETRA_OK) return fail("init shards", rc);
    if (one.setAachMinMargin(0) != TETRA_ERR_ARG || many.setAachMinMargin(931) != TETRA_ERR_ARG) return fail("min_margin outside 1..930", 0);
    if ((rc = one.setAachMinMargin(mm)) != TETRA_OK || (rc = many.setAachMinMargin(mm)) != TETRA_OK) return fail("setAachMinMargin", rc);
    long long rows = 0, refused = 0;
    for (int k = 0; k < calls; k++) {
        if (std::fread(iq.data(), sizeof(float), iq.size(), in) != iq.size()) return fail("short input", k);
        if ((rc = plain.process(N, iq.data())) != TETRA_OK) return fail("process soft-only", rc);
        if ((rc = one.process(N, iq.data())) != TETRA_OK) return fail("process", rc);
        if ((rc = many.process(N, iq.data())) != TETRA_OK) return fail("process shards", rc);
        TetraRxBank::Blocks p, a, b;
        std::vector<uint16_t> ma, mb;
        if ((rc = plain.fetch(TETRA_RX_KIND_BBK, p)) != TETRA_OK || (rc = one.fetch(TETRA_RX_KIND_BBK, a)) != TETRA_OK ||
            (rc = many.fetch(TETRA_RX_KIND_BBK, b)) != TETRA_OK)
            return fail("fetch", rc);
        if ((rc = one.fetchAachMargin(ma)) != TETRA_OK || (rc = many.fetchAachMargin(mb)) != TETRA_OK) return fail("fetchAachMargin", rc);
        if (ma.size() != a.info.size() || mb.size() != b.info.size() || ma.size() != mb.size() || p.info.size() != a.info.size()) return fail("row counts differ", k);
        if (a.type1 != b.type1) return fail("the shards' bits differ", k);
        for (size_t r = 0; r < ma.size(); r++) {
            if (ma[r] != mb[r] || a.info[r].channel != b.info[r].channel || a.info[r].bitnum != b.info[r].bitnum || a.info[r].crc_ok != b.info[r].crc_ok)
                return fail("rows differ", (long long)r);
            if (ma[r] > 255 || (a.info[r].crc_ok != 0) != (ma[r] >= mm)) return fail("margin and verdict disagree", (long long)r);
            if (p.info[r].channel != a.info[r].channel || p.info[r].bitnum != a.info[r].bitnum || p.info[r].crc_ok != 1) return fail("rows differ from the soft-only bank's", (long long)r);
            refused += a.info[r].crc_ok == 0;
        }
        rows += (long long)ma.size();
    }
    std::fclose(in);
    std::printf("test_aach_soft_bank: ok rows %lld refused %lld\n", rows, refused);
    return 0;
}
