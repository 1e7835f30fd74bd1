// test_sync_tol_bank.cpp -- TetraRxBank::setSyncTolerance / syncMisses (host/tetra_rx_bank.h) on a GPU (TEST TOOL, plain build).
//   test_sync_tol_bank <C> <N> <calls> <iq.bin>
// streams <calls> blocks of C x N complex64 samples (channel major, one after the other in the file) through three banks: one created
// with TETRA_RX_FLAG_SYNC_TOLERANT, one created without it and switched with setSyncTolerance({3, 5, 16}) before its first call, and
// one that stays with the reference's rule.  The first two must give the same rows of every kind after every call and the same miss
// counters; the third's SCH/F row count is printed beside theirs.  Values out of range are refused and change nothing; NULL returns
// a bank to the reference's rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tetra_rx_bank.h"

using dsp::demod::TetraRxBank;

static int fail(const char* what, long long v) { std::fprintf(stderr, "test_sync_tol_bank: %s (%lld)\n", what, v); return 1; }

int main(int argc, char** argv) {
    if (argc != 5) return fail("usage", argc);
    const int C = std::atoi(argv[1]), N = std::atoi(argv[2]), calls = std::atoi(argv[3]);
    std::vector<float> iq((size_t)2 * C * N);
    std::FILE* in = std::fopen(argv[4], "rb");
    if (!in) return fail("input file", 0);
    tetra_rx_config_t cfg;
    tetra_rx_default_config(&cfg);
    cfg.demod.n_channels = C;
    cfg.demod.max_samples = N;
    TetraRxBank flagged, set, plain;
    int rc;
    if ((rc = set.init(cfg)) != TETRA_OK || (rc = plain.init(cfg)) != TETRA_OK) return fail("init", rc);
    cfg.flags = TETRA_RX_FLAG_SYNC_TOLERANT;
    if ((rc = flagged.init(cfg)) != TETRA_OK) return fail("init with the flag", rc);
    const tetra_bsync_tolerance_t tol = { TETRA_SYNC_TOL_DEFAULT_NORM, TETRA_SYNC_TOL_DEFAULT_SYNC, TETRA_SYNC_TOL_DEFAULT_MISS };
    const tetra_bsync_tolerance_t bad[3] = { { 5, 0, 1 }, { 0, 7, 1 }, { 0, 0, 0 } };
    if ((rc = set.setSyncTolerance(&tol)) != TETRA_OK) return fail("setSyncTolerance", rc);
    for (const auto& b : bad)
        if (set.setSyncTolerance(&b) != TETRA_ERR_ARG) return fail("a tolerance out of range was accepted", b.tol_norm);
    long long rows = 0, schf_tol = 0, schf_plain = 0;
    std::vector<int32_t> ma, mb;
    for (int k = 0; k < calls; k++) {
        if (std::fread(iq.data(), sizeof(float), iq.size(), in) != iq.size()) return fail("short input", k);
        if ((rc = flagged.process(N, iq.data())) != TETRA_OK || (rc = set.process(N, iq.data())) != TETRA_OK || (rc = plain.process(N, iq.data())) != TETRA_OK)
            return fail("process", rc);
        for (int kind = 0; kind < TETRA_RX_N_KINDS; kind++) {
            TetraRxBank::Blocks a, b, p;
            if ((rc = flagged.fetch(kind, a)) != TETRA_OK || (rc = set.fetch(kind, b)) != TETRA_OK || (rc = plain.fetch(kind, p)) != TETRA_OK) return fail("fetch", rc);
            if (a.info.size() != b.info.size() || a.type1 != b.type1) return fail("rows differ", kind);
            for (size_t r = 0; r < a.info.size(); r++)
                if (std::memcmp(&a.info[r], &b.info[r], sizeof(a.info[r])) != 0) return fail("labels differ", kind);
            rows += (long long)a.info.size();
            if (kind == TETRA_RX_KIND_SCH_F) { schf_tol += (long long)a.info.size(); schf_plain += (long long)p.info.size(); }
        }
        if ((rc = flagged.syncMisses(ma)) != TETRA_OK || (rc = set.syncMisses(mb)) != TETRA_OK) return fail("syncMisses", rc);
        if ((int)ma.size() != C || ma != mb) return fail("miss counters differ", k);
        for (int32_t m : ma)
            if (m < 0 || m >= TETRA_SYNC_TOL_DEFAULT_MISS) return fail("a miss counter out of range", m);
    }
    if ((rc = set.setSyncTolerance(nullptr)) != TETRA_OK) return fail("setSyncTolerance(NULL)", rc);
    if ((rc = set.syncMisses(mb)) != TETRA_OK) return fail("syncMisses", rc);
    for (int32_t m : mb)
        if (m != 0) return fail("setting did not zero a miss counter", m);
    if ((rc = flagged.wait()) != TETRA_OK || (rc = set.wait()) != TETRA_OK || (rc = plain.wait()) != TETRA_OK) return fail("wait", rc);
    std::fclose(in);
    std::printf("test_sync_tol_bank: ok %lld rows %lld schf %lld schf_plain\n", rows, schf_tol, schf_plain);
    return 0;
}
