// test_gap_bank.cpp -- TetraRxBank::resume and its TetraRxMultiBank forwarding (host/tetra_rx_bank.h; include/ext/tetra_gap.h): a plain
// C++ driver for tests/test_gap.py.  No samples are fed: every channel is UNLOCKED, so an accepted resume reads REFUSED for the listed
// channels and NONE for the others, and what the forwarding refuses changes nothing.
//   test_gap_bank <channels> <shards>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int C = std::atoi(argv[1]), G = std::atoi(argv[2]);
    tetra_rx_config_t cfg;
    CHECK(tetra_rx_default_config(&cfg) == TETRA_OK);
    cfg.demod.n_channels = C;
    cfg.demod.max_samples = 1024;
    cfg.kinds = 1 << TETRA_RX_KIND_SB1;
    TetraRxMultiBank multi;
    CHECK(multi.init(cfg, std::vector<int>((size_t)G, 0)) == TETRA_OK);
    int first1 = 0, count1 = 0;
    multi.shardInfo(1, first1, count1);
    CHECK(first1 >= 2 && count1 >= 2);
    std::vector<tetra_handover_status_t> st;
    // a channel outside the bank, one listed twice, elapsed bits and parameters out of range
    const tetra_handover_params_t bad = { 8, 256 };
    CHECK(multi.resume({ C }, 137) == TETRA_ERR_ARG && multi.resume({ -1 }, 137) == TETRA_ERR_ARG);
    CHECK(multi.resume({ 1, first1, 1 }, 137) == TETRA_ERR_ARG);
    CHECK(multi.resume({ 1 }, -1) == TETRA_ERR_ARG && multi.resume({ 1 }, (int64_t)TETRA_GAP_MAX_ELAPSED_BITS + 1) == TETRA_ERR_ARG);
    CHECK(multi.resume({ 1 }, 137, &bad) == TETRA_ERR_ARG);
    CHECK(multi.handoverStatus(st) == TETRA_OK && (int)st.size() == C);
    for (const auto& s : st) CHECK(s.state == TETRA_HANDOVER_NONE && s.slots_waited == 0 && s.offset == 0);
    // accepted: one channel of shard 0, two of shard 1, in the bank's numbering
    CHECK(multi.resume({ first1 + 1, 1, first1 }, TETRA_GAP_MAX_ELAPSED_BITS) == TETRA_OK);
    CHECK(multi.handoverStatus(st) == TETRA_OK && (int)st.size() == C);
    for (int c = 0; c < C; c++) CHECK(st[(size_t)c].state == ((c == 1 || c == first1 || c == first1 + 1) ? TETRA_HANDOVER_REFUSED : TETRA_HANDOVER_NONE));
    // an empty list is accepted and changes nothing; the single bank answers like a shard
    CHECK(multi.resume({}, 5) == TETRA_OK);
    TetraRxBank& one = multi.shard(1);
    std::vector<tetra_handover_status_t> s1;
    CHECK(one.handoverStatus(s1) == TETRA_OK && (int)s1.size() == count1 && s1[0].state == TETRA_HANDOVER_REFUSED && s1[1].state == TETRA_HANDOVER_REFUSED);
    CHECK(one.resume({ count1 }, 5) == TETRA_ERR_ARG && one.resume({ 0 }, -5) == TETRA_ERR_ARG);
    CHECK(one.resume({ 0 }, 0) == TETRA_OK);
    CHECK(multi.wait() == TETRA_OK);
    std::printf("test_gap_bank: ok\n");
    return 0;
}
