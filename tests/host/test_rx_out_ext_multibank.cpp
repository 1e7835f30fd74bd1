// test_rx_out_ext_multibank.cpp -- TetraRxMultiBank::fetchAll with extras (host/tetra_rx_bank.h, include/ext/tetra_rx_out_ext.h)
// against the blocking fetches and getters, on a GPU (TEST TOOL, plain build).
//   test_rx_out_ext_multibank <C> <N> <calls> <iq.bin> <shards> <flags>
// streams <calls> blocks of C x N complex64 samples (channel major, one after the other in the file) through a bank created with the
// bit-error counts, the list decoder, the AACH's Reed-Muller code and the tolerant lock, all shards on device 0, the snapshot armed.
// After each call the previous call's rows and columns (which = 1, while this call runs) and at the end the last call's (which = 0)
// come over both ways; they must be equal row for row (with TETRA_RX_OUT_CRC_GOOD: the fetched rows with crc_ok != 0).  The last
// call's per-channel tables must equal the blocking getters', which answer with the state behind the latest tail.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_aach.h"
#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;
using dsp::demod::TetraRxMultiBank;

static int fail(const char* what, long long v) { std::fprintf(stderr, "test_rx_out_ext_multibank: %s (%lld)\n", what, v); return 1; }

static const int kEvery = TETRA_RX_OUT_EXT_ROW_ALL | TETRA_RX_OUT_EXT_CHAN_ALL;

// the shards' AACH distances one after the other, as fetchAll concatenates them
static int fetchAachDist(TetraRxMultiBank& bank, std::vector<uint8_t>& out, int which) {
    out.clear();
    for (int s = 0; s < bank.shards(); s++) {
        int n = 0;
        int rc = tetra_rx_fetch_aach_dist(bank.shard(s).handle(), which, nullptr, 0, &n);
        if (rc != TETRA_OK) return rc;
        std::vector<uint8_t> part((size_t)n);
        if (n && (rc = tetra_rx_fetch_aach_dist(bank.shard(s).handle(), which, part.data(), n, &n)) != TETRA_OK) return rc;
        out.insert(out.end(), part.begin(), part.end());
    }
    return TETRA_OK;
}

template <typename T> static bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0);
}

static long long compare(TetraRxMultiBank& bank, int which, int flags, int& bad, long long& nonzero) {
    TetraRxBank::Blocks all[TETRA_RX_N_KINDS];
    TetraRxBank::Channels chans;
    int rc = bank.fetchAll(all, which, 0, flags, kEvery, &chans);
    if (rc != TETRA_OK) { bad = rc; return 0; }
    long long rows = 0;
    for (int k = 0; k < TETRA_RX_N_KINDS; k++) {
        TetraRxBank::Blocks want;
        if ((rc = bank.fetch(k, want, which)) != TETRA_OK) { bad = rc; return 0; }
        std::vector<uint32_t> be;
        std::vector<int32_t> rk;
        std::vector<uint8_t> ad;
        if (k == TETRA_RX_KIND_BBK) rc = fetchAachDist(bank, ad, which);
        else if ((rc = bank.fetchBitErrors(k, be, which)) == TETRA_OK) rc = bank.fetchListRank(k, rk, which);
        if (rc != TETRA_OK) { bad = rc; return 0; }
        std::vector<size_t> keep;
        for (size_t r = 0; r < want.info.size(); r++)
            if (!(flags & TETRA_RX_OUT_CRC_GOOD) || want.info[r].crc_ok) keep.push_back(r);
        const bool bbk = k == TETRA_RX_KIND_BBK;
        if (all[k].info.size() != keep.size() || all[k].biterr.size() != (bbk ? 0 : keep.size()) || all[k].rank.size() != (bbk ? 0 : keep.size()) ||
            all[k].aachDist.size() != (bbk ? keep.size() : 0)) { bad = 100 + k; return 0; }
        for (size_t i = 0; i < keep.size(); i++) {
            const size_t r = keep[i];
            if (std::memcmp(&all[k].info[i], &want.info[r], sizeof(tetra_rx_block_t)) != 0) { bad = 200 + k; return 0; }
            if (bbk ? all[k].aachDist[i] != ad[r] : (all[k].biterr[i] != be[r] || all[k].rank[i] != rk[r])) { bad = 300 + k; return 0; }
            nonzero += bbk ? (ad[r] != 0) : ((be[r] & 0xffffu) != 0) + (rk[r] != 0);
        }
        rows += (long long)keep.size();
    }
    if ((int)chans.cell.size() != bank.channels() || (int)chans.sync.size() != bank.channels() || (int)chans.misses.size() != bank.channels() ||
        (int)chans.link.size() != bank.channels()) { bad = 400; return 0; }
    if (which == 0) {
        TetraRxBank::Channels want;
        if ((rc = bank.cells(want.cell)) != TETRA_OK || (rc = bank.syncStates(want.sync)) != TETRA_OK || (rc = bank.syncMisses(want.misses)) != TETRA_OK ||
            (rc = bank.links(want.link)) != TETRA_OK) { bad = rc; return 0; }
        if (!same(chans.cell, want.cell)) { bad = 401; return 0; }
        if (!same(chans.sync, want.sync)) { bad = 402; return 0; }
        if (!same(chans.misses, want.misses)) { bad = 403; return 0; }
        if (!same(chans.link, want.link)) { bad = 404; return 0; }
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
    cfg.flags = TETRA_RX_FLAG_BITERR | TETRA_RX_FLAG_LIST | TETRA_RX_FLAG_AACH_RM3014 | TETRA_RX_FLAG_SYNC_TOLERANT;
    TetraRxMultiBank bank;
    int rc = bank.init(cfg, std::vector<int>((size_t)shards, 0));
    if (rc != TETRA_OK) return fail("init", rc);
    if ((rc = bank.setSnapshot(TETRA_RX_OUT_EXT_CHAN_ALL)) != TETRA_OK) return fail("setSnapshot", rc);
    long long rows = 0, nonzero = 0;
    int bad = 0;
    for (int k = 0; k < calls; k++) {
        if (std::fread(iq.data(), sizeof(float), iq.size(), in) != iq.size()) return fail("short input", k);
        if ((rc = bank.process(N, iq.data())) != TETRA_OK) return fail("process", rc);
        if (k >= 1) {
            rows += compare(bank, 1, flags, bad, nonzero);
            if (bad) return fail("previous call differs", bad);
        }
    }
    rows += compare(bank, 0, flags, bad, nonzero);
    if (bad) return fail("last call differs", bad);
    if ((rc = bank.wait()) != TETRA_OK) return fail("wait", rc);
    if (nonzero == 0) return fail("every column is zero", 0);
    std::fclose(in);
    std::printf("test_rx_out_ext_multibank: ok %lld rows\n", rows);
    return 0;
}
