// test_traffic_bank.cpp -- TetraRxBank::enableTraffic / setTraffic / fetchTraffic and their TetraRxMultiBank forms (host/tetra_rx_bank.h;
// include/ext/tetra_traffic.h): a plain C++ driver for tests/test_rx_traffic_gpu.py.  The same samples and table through one bank and
// through <shards> shards on one GPU: the shards' rows, one after the other, are the single bank's -- labels in the bank's channel
// numbers, bits and count words -- and a table range outside the bank is refused.  Prints the rows per kind for the caller.
//   test_traffic_bank <channels> <shards> <samples> <iq file: complex64 [channels][samples]> <table file: [channels][4][4 bytes]>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

template <class T> static bool read_file(const char* path, std::vector<T>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t n = std::fread(out.data(), sizeof(T), out.size(), f);
    std::fclose(f);
    return n == out.size();
}

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const int C = std::atoi(argv[1]), G = std::atoi(argv[2]), N = std::atoi(argv[3]);
    std::vector<float> iq((size_t)2 * C * N);
    std::vector<tetra_rx_traffic_slot_t> table((size_t)4 * C);
    CHECK(read_file(argv[4], iq) && read_file(argv[5], table));
    tetra_rx_config_t cfg;
    CHECK(tetra_rx_default_config(&cfg) == TETRA_OK);
    cfg.demod.n_channels = C;
    cfg.demod.max_samples = N;
    cfg.flags = TETRA_RX_FLAG_BITERR;
    TetraRxBank one;
    TetraRxMultiBank multi;
    CHECK(one.init(cfg) == TETRA_OK && multi.init(cfg, std::vector<int>((size_t)G, 0)) == TETRA_OK);
    TetraRxBank::Blocks a, b;
    CHECK(one.fetchTraffic(TETRA_LMAC_T_TCH_4_8, a) == TETRA_ERR_UNSUPPORTED && multi.fetchTraffic(TETRA_LMAC_T_TCH_4_8, a) == TETRA_ERR_UNSUPPORTED);
    CHECK(one.enableTraffic() == TETRA_OK && multi.enableTraffic() == TETRA_OK);
    CHECK(multi.setTraffic(1, table) == TETRA_ERR_ARG && multi.setTraffic(-1, {}) == TETRA_ERR_ARG);
    CHECK(multi.setTraffic(0, std::vector<tetra_rx_traffic_slot_t>(3)) == TETRA_ERR_ARG);
    // the table in two pieces that do not end on a shard's edge
    const std::vector<tetra_rx_traffic_slot_t> head(table.begin(), table.begin() + 4), rest(table.begin() + 4, table.end());
    CHECK(one.setTraffic(0, table) == TETRA_OK && multi.setTraffic(1, rest) == TETRA_OK && multi.setTraffic(0, head) == TETRA_OK);
    CHECK(one.process(N, iq.data()) == TETRA_OK && multi.process(N, iq.data()) == TETRA_OK);
    int total = 0;
    for (int kind = TETRA_LMAC_T_TCH_7_2; kind <= TETRA_LMAC_T_TCH_2_4; kind++) {
        int da = -1, db = -1;
        CHECK(one.fetchTraffic(kind, a, &da) == TETRA_OK && multi.fetchTraffic(kind, b, &db) == TETRA_OK && da == 0 && db == 0);
        CHECK(a.info.size() == b.info.size() && a.bitsPerBlock == b.bitsPerBlock && a.type1 == b.type1 && a.biterr == b.biterr);
        CHECK(a.biterr.size() == (kind == TETRA_LMAC_T_TCH_7_2 ? 0 : a.info.size()));
        for (size_t j = 0; j < a.info.size(); j++) {
            const tetra_rx_block_t &x = a.info[j], &y = b.info[j];
            CHECK(x.channel == y.channel && x.bitnum == y.bitnum && x.tdma_time == y.tdma_time && x.tdma_time_rx == y.tdma_time_rx && x.crc_ok == 1 && y.crc_ok == 1);
            CHECK(j == 0 || x.channel > a.info[j - 1].channel || (x.channel == a.info[j - 1].channel && x.bitnum > a.info[j - 1].bitnum));
        }
        std::printf("rows %d %zu\n", kind, a.info.size());
        total += (int)a.info.size();
    }
    CHECK(total > 0);
    // a small maxRows on a second multi-bank: every shard keeps its own first rows, the rest is counted
    TetraRxMultiBank small;
    CHECK(small.init(cfg, std::vector<int>((size_t)G, 0)) == TETRA_OK && small.enableTraffic(1) == TETRA_OK && small.setTraffic(0, table) == TETRA_OK);
    CHECK(small.process(N, iq.data()) == TETRA_OK);
    int dropped = -1;
    CHECK(one.fetchTraffic(TETRA_LMAC_T_TCH_4_8, a) == TETRA_OK && small.fetchTraffic(TETRA_LMAC_T_TCH_4_8, b, &dropped) == TETRA_OK);
    CHECK((int)b.info.size() <= G && (int)b.info.size() + dropped == (int)a.info.size());
    CHECK(one.wait() == TETRA_OK && multi.wait() == TETRA_OK && small.wait() == TETRA_OK);
    std::printf("test_traffic_bank: ok\n");
    return 0;
}
