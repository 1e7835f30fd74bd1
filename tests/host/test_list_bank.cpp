// test_list_bank.cpp -- TetraRxBank::setListCandidates / fetchListRank and their TetraRxMultiBank concatenation (host/tetra_rx_bank.h)
// on a GPU (TEST TOOL, plain build).
//   test_list_bank <C> <N> <calls> <iq.bin> <shards>
// streams <calls> blocks of C x N complex64 samples (channel major, one after the other in the file) through ONE bank of C channels
// and through a bank of <shards> shards on device 0, both with TETRA_RX_FLAG_LIST and eight candidates, and through a bank without the
// flag.  After every call the shards' ranks, one after the other, must be the single bank's, row for row beside fetch()'s rows; a rank
// says what the row's verdict is (>= 0: good), and against the bank without the flag no good block is lost.
// Prints: test_list_bank: ok rows <n> rescued <n>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

static int fail(const char* what, long long v) { std::fprintf(stderr, "test_list_bank: %s (%lld)\n", what, v); return 1; }

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
    TetraRxBank plain, one;
    TetraRxMultiBank many;
    int rc = plain.init(cfg);
    if (rc != TETRA_OK) return fail("init plain", rc);
    std::vector<int32_t> none;
    if (plain.setListCandidates(4) != TETRA_ERR_UNSUPPORTED || plain.fetchListRank(TETRA_RX_KIND_SCH_F, none) != TETRA_ERR_UNSUPPORTED)
        return fail("without the flag", 0);
    cfg.flags = TETRA_RX_FLAG_LIST;
    if ((rc = one.init(cfg)) != TETRA_OK) return fail("init", rc);
    if ((rc = many.init(cfg, std::vector<int>((size_t)shards, 0))) != TETRA_OK) return fail("init shards", rc);
    if (one.setListCandidates(0) != TETRA_ERR_ARG || many.setListCandidates(9) != TETRA_ERR_ARG) return fail("T outside 1..8", 0);
    if ((rc = one.setListCandidates(8)) != TETRA_OK || (rc = many.setListCandidates(8)) != TETRA_OK) return fail("setListCandidates", rc);
    long long rows = 0, rescued = 0;
    const int coded[5] = { TETRA_RX_KIND_SB1, TETRA_RX_KIND_SB2, TETRA_RX_KIND_NDB1, TETRA_RX_KIND_NDB2, TETRA_RX_KIND_SCH_F };
    for (int k = 0; k < calls; k++) {
        if (std::fread(iq.data(), sizeof(float), iq.size(), in) != iq.size()) return fail("short input", k);
        if ((rc = plain.process(N, iq.data())) != TETRA_OK) return fail("process plain", rc);
        if ((rc = one.process(N, iq.data())) != TETRA_OK) return fail("process", rc);
        if ((rc = many.process(N, iq.data())) != TETRA_OK) return fail("process shards", rc);
        for (int kind : coded) {
            TetraRxBank::Blocks p, a, b;
            std::vector<int32_t> ra, rb;
            if ((rc = plain.fetch(kind, p)) != TETRA_OK || (rc = one.fetch(kind, a)) != TETRA_OK || (rc = many.fetch(kind, b)) != TETRA_OK) return fail("fetch", rc);
            if ((rc = one.fetchListRank(kind, ra)) != TETRA_OK || (rc = many.fetchListRank(kind, rb)) != TETRA_OK) return fail("fetchListRank", rc);
            if (ra.size() != a.info.size() || rb.size() != b.info.size() || ra.size() != rb.size() || p.info.size() != a.info.size()) return fail("row counts differ", kind);
            for (size_t r = 0; r < ra.size(); r++) {
                if (ra[r] != rb[r] || a.info[r].channel != b.info[r].channel || a.info[r].bitnum != b.info[r].bitnum) return fail("rows differ", kind);
                if (ra[r] < -1 || ra[r] > 8 || (ra[r] >= 0) != (a.info[r].crc_ok != 0)) return fail("rank and verdict disagree", kind);
                if (p.info[r].channel != a.info[r].channel || p.info[r].bitnum != a.info[r].bitnum) return fail("rows differ from the plain bank's", kind);
                // (a block decoded under a code that only a rescued SB1 supplied may be good where the plain bank's is not: never the reverse
                // for the rows the decoder itself passes under the same code, so only SB1 -- always under the fixed code -- is held to it)
                if (kind == TETRA_RX_KIND_SB1 && p.info[r].crc_ok && ra[r] != 0) return fail("a good SB1 was touched", (long long)r);
                rescued += ra[r] > 0;
            }
            rows += (long long)ra.size();
        }
        if (one.fetchListRank(TETRA_RX_KIND_BBK, none) != TETRA_ERR_UNSUPPORTED) return fail("the AACH has no ranks", k);
    }
    std::fclose(in);
    std::printf("test_list_bank: ok rows %lld rescued %lld\n", rows, rescued);
    return 0;
}
