// test_handover_bank.cpp -- TetraRxBank::handOver / handoverStatus and their TetraRxMultiBank forwarding (host/tetra_rx_bank.h;
// include/ext/tetra_handover.h): a plain C++ driver for tests/test_handover.py.  No samples are fed: every donor is UNLOCKED, so an accepted
// hand-over reads REFUSED, a plain restart NONE, and what the forwarding refuses changes nothing.
//   test_handover_bank <channels> <shards>
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
    CHECK(multi.handoverStatus(st) == TETRA_OK && (int)st.size() == C);
    for (const auto& s : st) CHECK(s.state == TETRA_HANDOVER_NONE && s.slots_waited == 0 && s.offset == 0);
    // donor and heir in different shards, a channel outside the bank, lists of different lengths, a donor that is an heir, bad parameters
    const tetra_handover_params_t bad = { 128, 72 };
    CHECK(multi.handOver({ 1 }, { first1 }) == TETRA_ERR_ARG);
    CHECK(multi.handOver({ first1 }, { 0 }) == TETRA_ERR_ARG);
    CHECK(multi.handOver({ C }, { 0 }) == TETRA_ERR_ARG && multi.handOver({ -1 }, { 0 }) == TETRA_ERR_ARG);
    CHECK(multi.handOver({ 0, 1 }, { 1 }) == TETRA_ERR_ARG);
    CHECK(multi.handOver({ 0, 1 }, { 1, -1 }) == TETRA_ERR_ARG);
    CHECK(multi.handOver({ 1 }, { 0 }, &bad) == TETRA_ERR_ARG);
    CHECK(multi.handoverStatus(st) == TETRA_OK);
    for (const auto& s : st) CHECK(s.state == TETRA_HANDOVER_NONE);
    // accepted: heir 1 from donor 0 (shard 0), heir first1 + 1 from donor first1 (shard 1), channel first1 - 1 restarted plainly
    CHECK(multi.handOver({ 1, first1 + 1, first1 - 1 }, { 0, first1, -1 }) == TETRA_OK);
    CHECK(multi.handoverStatus(st) == TETRA_OK && (int)st.size() == C);
    for (int c = 0; c < C; c++) CHECK(st[(size_t)c].state == ((c == 1 || c == first1 + 1) ? TETRA_HANDOVER_REFUSED : TETRA_HANDOVER_NONE));
    // a plain restart of an heir clears its status; the single bank answers like a shard
    CHECK(multi.handOver({ 1 }, { -1 }) == TETRA_OK && multi.handoverStatus(st) == TETRA_OK && st[1].state == TETRA_HANDOVER_NONE);
    TetraRxBank& one = multi.shard(1);
    std::vector<tetra_handover_status_t> s1;
    CHECK(one.handoverStatus(s1) == TETRA_OK && (int)s1.size() == count1 && s1[1].state == TETRA_HANDOVER_REFUSED);
    CHECK(one.handOver({ 0 }, { count1 }) == TETRA_ERR_ARG && one.handOver({ 0 }, { 1, 1 }) == TETRA_ERR_ARG);
    CHECK(multi.wait() == TETRA_OK);
    std::printf("test_handover_bank: ok\n");
    return 0;
}
