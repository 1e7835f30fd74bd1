// test_rx_out_multibank.cpp -- TetraRxMultiBank::fetchAll (host/tetra_rx_bank.h: every shard's delivery enqueued, then collected)
// against fetch() of each kind, on a GPU (TEST TOOL, plain build).
//   test_rx_out_multibank <C> <N> <calls> <iq.bin> <shards> <flags>
// streams <calls> blocks of C x N complex64 samples (channel major, one after the other in the file) through the bank, all shards on
// device 0.  After each call the previous call's blocks (which = 1, while this call runs) and at the end the last call's blocks
// (which = 0) come over both ways; they must be equal row for row (with TETRA_RX_OUT_CRC_GOOD: fetch's rows with crc_ok != 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

static int fail(const char* what, long long v) { std::fprintf(stderr, "test_rx_out_multibank: %s (%lld)\n", what, v); return 1; }

static long long compare(TetraRxMultiBank& bank, int which, int flags, int& bad) {
    TetraRxBank::Blocks all[TETRA_RX_N_KINDS];
    int rc = bank.fetchAll(all, which, 0, flags);
    if (rc != TETRA_OK) { bad = rc; return 0; }
    long long rows = 0;
    for (int k = 0; k < TETRA_RX_N_KINDS; k++) {
        TetraRxBank::Blocks want;
        if ((rc = bank.fetch(k, want, which)) != TETRA_OK) { bad = rc; return 0; }
        const int nb = want.bitsPerBlock;
        std::vector<size_t> keep;
        for (size_t r = 0; r < want.info.size(); r++)
            if (!(flags & TETRA_RX_OUT_CRC_GOOD) || want.info[r].crc_ok) keep.push_back(r);
        if (all[k].info.size() != keep.size() || all[k].bitsPerBlock != nb) { bad = 100 + k; return 0; }
        for (size_t i = 0; i < keep.size(); i++) {
            if (std::memcmp(&all[k].info[i], &want.info[keep[i]], sizeof(tetra_rx_block_t)) != 0 ||
                std::memcmp(all[k].bits(i), want.bits(keep[i]), (size_t)nb) != 0) {
                bad = 200 + k;
                return 0;
            }
        }
        rows += (long long)keep.size();
    }
    return rows;
}

int main(int argc, char** argv) {
    if (argc != 7) return fail("usage", argc);
    const int C = std::atoi(argv[1]), N = std::atoi(argv[2]), calls = std::atoi(argv[3]), shards = std::atoi(argv[5]), flags = std::atoi(argv[6]);
    std::vector<float> iq((size_t)2 * C * N);
    std::FILE* in = std::fopen(argv[4], "rb");
    if (!in) return fail("input file", 0);
    tetra_rx_config_t cfg;
    tetra_rx_default_config(&cfg);
    cfg.demod.n_channels = C;
    cfg.demod.max_samples = N;
    TetraRxMultiBank bank;
    int rc = bank.init(cfg, std::vector<int>((size_t)shards, 0));
    if (rc != TETRA_OK) return fail("init", rc);
    long long rows = 0;
    int bad = 0;
    for (int k = 0; k < calls; k++) {
        if (std::fread(iq.data(), sizeof(float), iq.size(), in) != iq.size()) return fail("short input", k);
        if ((rc = bank.process(N, iq.data())) != TETRA_OK) return fail("process", rc);
        if (k >= 1) {
            rows += compare(bank, 1, flags, bad);
            if (bad) return fail("previous call differs", bad);
        }
    }
    rows += compare(bank, 0, flags, bad);
    if (bad) return fail("last call differs", bad);
    if ((rc = bank.wait()) != TETRA_OK) return fail("wait", rc);
    std::fclose(in);
    std::printf("test_rx_out_multibank: ok %lld rows\n", rows);
    return 0;
}
