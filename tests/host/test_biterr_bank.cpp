// test_biterr_bank.cpp -- TetraRxBank::fetchBitErrors / links and their TetraRxMultiBank concatenation (host/tetra_rx_bank.h) on a
// GPU (TEST TOOL, plain build).
//   test_biterr_bank <C> <N> <calls> <iq.bin> <shards>
// streams <calls> blocks of C x N complex64 samples (channel major, one after the other in the file) through ONE bank of C channels
// and through a bank of <shards> shards on device 0, both with TETRA_RX_FLAG_BITERR.  After every call the shards' counts, one after
// the other, must be the single bank's, row for row beside fetch()'s rows; at the end the shards' link figures in channel order must be
// the single bank's, and those must be the sums of its own rows over all calls.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

static int fail(const char* what, long long v) { std::fprintf(stderr, "test_biterr_bank: %s (%lld)\n", what, v); return 1; }

int main(int argc, char** argv) {
    if (argc != 6) return fail("usage", argc);
    const int C = std::atoi(argv[1]), N = std::atoi(argv[2]), calls = std::atoi(argv[3]), shards = std::atoi(argv[5]);
    std::vector<float> iq((size_t)2 * C * N);
    std::FILE* in = std::fopen(argv[4], "rb");
    if (!in) return fail("input file", 0);
    tetra_rx_config_t cfg;
    tetra_rx_default_config(&cfg);
    cfg.demod.n_channels = C;
    cfg.demod.max_samples = N;
    cfg.flags = TETRA_RX_FLAG_BITERR;
    TetraRxBank one;
    TetraRxMultiBank many;
    int rc = one.init(cfg);
    if (rc != TETRA_OK) return fail("init", rc);
    if ((rc = many.init(cfg, std::vector<int>((size_t)shards, 0))) != TETRA_OK) return fail("init shards", rc);
    std::vector<tetra_rx_link_t> sums((size_t)C);
    std::memset(sums.data(), 0, sizeof(tetra_rx_link_t) * sums.size());
    long long rows = 0;
    const int coded[5] = { TETRA_RX_KIND_SB1, TETRA_RX_KIND_SB2, TETRA_RX_KIND_NDB1, TETRA_RX_KIND_NDB2, TETRA_RX_KIND_SCH_F };
    for (int k = 0; k < calls; k++) {
        if (std::fread(iq.data(), sizeof(float), iq.size(), in) != iq.size()) return fail("short input", k);
        if ((rc = one.process(N, iq.data())) != TETRA_OK) return fail("process", rc);
        if ((rc = many.process(N, iq.data())) != TETRA_OK) return fail("process shards", rc);
        for (int kind : coded) {
            TetraRxBank::Blocks a, b;
            std::vector<uint32_t> ea, eb;
            if ((rc = one.fetch(kind, a)) != TETRA_OK || (rc = many.fetch(kind, b)) != TETRA_OK) return fail("fetch", rc);
            if ((rc = one.fetchBitErrors(kind, ea)) != TETRA_OK || (rc = many.fetchBitErrors(kind, eb)) != TETRA_OK) return fail("fetchBitErrors", rc);
            if (ea.size() != a.info.size() || eb.size() != b.info.size() || ea.size() != eb.size()) return fail("row counts differ", kind);
            for (size_t r = 0; r < ea.size(); r++) {
                if (ea[r] != eb[r] || a.info[r].channel != b.info[r].channel || a.info[r].bitnum != b.info[r].bitnum) return fail("rows differ", kind);
                tetra_rx_link_t& l = sums[(size_t)a.info[r].channel];
                l.blocks++;
                if (a.info[r].crc_ok) { l.bits += TETRA_BITERR_COMPARED(ea[r]); l.bit_errors += TETRA_BITERR_ERRORS(ea[r]); }
                else l.blocks_crc_bad++;
            }
            rows += (long long)ea.size();
        }
        std::vector<uint32_t> none;
        if (one.fetchBitErrors(TETRA_RX_KIND_BBK, none) != TETRA_ERR_UNSUPPORTED) return fail("the AACH has no counts", k);
    }
    std::vector<tetra_rx_link_t> la, lb;
    if ((rc = one.links(la)) != TETRA_OK || (rc = many.links(lb)) != TETRA_OK) return fail("links", rc);
    if ((int)la.size() != C || (int)lb.size() != C) return fail("link counts", (long long)lb.size());
    long long bad = 0;
    for (int c = 0; c < C; c++) {
        if (std::memcmp(&la[(size_t)c], &lb[(size_t)c], sizeof(tetra_rx_link_t)) != 0) return fail("shard links differ", c);
        if (la[(size_t)c].bits != sums[(size_t)c].bits || la[(size_t)c].bit_errors != sums[(size_t)c].bit_errors ||
            la[(size_t)c].blocks != sums[(size_t)c].blocks || la[(size_t)c].blocks_crc_bad != sums[(size_t)c].blocks_crc_bad)
            return fail("links are not the sums of the rows", c);
        bad += la[(size_t)c].blocks_crc_bad;
    }
    if ((rc = one.wait()) != TETRA_OK || (rc = many.wait()) != TETRA_OK) return fail("wait", rc);
    std::fclose(in);
    std::printf("test_biterr_bank: ok %lld rows %lld bad\n", rows, bad);
    return 0;
}
