"""TETRA_RX_FLAG_LIST through the receive chain (include/ext/tetra_list.h): the chain's rows, verdicts, times and ranks against
tests/list_pipeline.py -- the burst-synchroniser oracle's frames, every coded block decoded and rescued by the numpy definition, SB1
first and feeding the tracker's walk.  Four downlinks at Es/N0 = 11 dB from the synth fixtures, two calls of 9000 samples."""
import numpy as np
import pytest

from tests import chain_host as ch
from tests import list_pipeline as LP
from tests import soft_pipeline as sp
from tests.chain_gpu import device_bytes as _device_bytes, run_calls

SAMPLES, CUT, SLOTS, ESN0 = 18000, 9000, 36, 11.0
SEEDS = (214, 186, 259, 56)            # chosen so that rescued SB1s change later blocks (test_the_chosen_input_... checks it on the CPU)
ERR_UNSUPPORTED, ERR_ARG = -2, -1      # include/tetra_demod.h


@pytest.fixture(scope="module")
def iq(synth):
    rows = []
    for seed in SEEDS:
        tx = synth.gen_downlink(SLOTS, 8100 + seed, cell=(200 + seed % 50, 3000 + seed, 9 + seed % 40))
        rows.append(synth.gen_channel(SAMPLES, 8200 + seed, bits=tx[0], esn0_db=ESN0)[0])
    out = np.stack(rows).astype(np.complex64)
    out.flags.writeable = False
    return out


@pytest.fixture(scope="module")
def oracle_stream(oracle, iq):
    """the oracle demodulator's bits and quantised soft values per channel"""
    return sp.oracle_streams(oracle, np.array(iq))


def expected(oracle, bits, T, soft=None):
    want = {}
    for c in range(len(bits)):
        want.update(LP.channel_rows(oracle, bits[c], c, T, None if soft is None else soft[c]))
    return want


def test_the_chosen_input_holds_rescued_rows_and_a_rescued_sb1_that_matters(oracle, oracle_stream):
    """On the CPU, from the oracle demodulator's bits: with four candidates rows are rescued on both routes, no block is lost, and a block
    behind a rescued SB1 comes out with another verdict, other bits or another time than without the rescue (hard and soft)."""
    bits, soft = oracle_stream
    for sv in (None, soft):
        w, wo = expected(oracle, bits, 4, sv), expected(oracle, bits, 0, sv)
        assert set(w) == set(wo) and len(w) >= 80
        assert all(w[k][0] >= wo[k][0] for k in w) and all(v[4] == (0 if v[0] else -1) for v in wo.values())
        assert sum(v[4] > 0 for v in w.values()) >= 3 and any(k[0] == ch.KIND_SB1 and v[4] > 0 for k, v in w.items())
        assert any(v[4] == -1 for v in w.values())
        assert LP.rescued_sb1_matters(w, wo)


def run_chain(pkg, iq, flags, T=None):
    """the stream in two calls through one handle -> {(kind, channel, bitnum): (crc_ok, time on entry, time, type-1 bytes, rank, counts)}
    (rank None without FLAG_LIST, counts None without FLAG_BITERR), the AACH rows, the channels' bits, the cells"""
    import torch
    R = pkg.rx_binding
    rows, aach, ranks = {}, [], []

    def per_call(rx, i, s):
        for k in LP.CODED_KINDS:
            blocks, t1 = rx.fetch(k)
            rank = rx.fetch_list_rank(k) if flags & R.FLAG_LIST else [None] * len(blocks)
            err, cmp_ = rx.fetch_biterr(k) if flags & R.FLAG_BITERR else ([None] * len(blocks), [None] * len(blocks))
            assert len(rank) == len(blocks)
            ranks.append(rank)
            if flags & R.FLAG_LIST and len(blocks):
                dr = _device_bytes(torch, rx.list_rank_device(k, 0, s), (len(blocks),), "<i4").cpu().numpy()
                assert np.array_equal(dr, rank)
            for j, blk in enumerate(blocks):
                key = (k, int(blk["channel"]), int(blk["bitnum"]))
                assert key not in rows
                rows[key] = (int(blk["crc_ok"]), int(blk["tdma_time_rx"]), int(blk["tdma_time"]), t1[j].tobytes(),
                             None if rank[j] is None else int(rank[j]), None if err[j] is None else (int(err[j]), int(cmp_[j])))
        blocks, t1 = rx.fetch(R.KIND_BBK)
        aach.append((blocks.tobytes(), t1.tobytes()))

    def after(rx):
        if flags & R.FLAG_LIST:        # the rank buffers are double buffered like the results: which = 1 is the first call's
            s = torch.cuda.current_stream()
            for j, k in enumerate(LP.CODED_KINDS):
                first, second = ranks[j], ranks[len(LP.CODED_KINDS) + j]
                assert np.array_equal(rx.fetch_list_rank(k, which=1), first) and np.array_equal(rx.fetch_list_rank(k, which=0), second)
                if len(first):
                    assert np.array_equal(_device_bytes(torch, rx.list_rank_device(k, 1, s), (len(first),), "<i4").cpu().numpy(), first)

    bits, cells, _ = run_calls(pkg, iq, (0, CUT, SAMPLES), flags, per_call, None if T is None else lambda rx: rx.set_list_candidates(T), after)
    return rows, aach, bits, cells


@pytest.mark.gpu
@pytest.mark.parametrize("route", ("hard", "one_stream", "soft", "soft_biterr"))
def test_gpu_chain_equals_the_pipeline_on_every_row(pkg, oracle, oracle_stream, iq, route):
    """The chain with FLAG_LIST (two streams, one stream, with FLAG_SOFT, with FLAG_SOFT | FLAG_BITERR) equals the pipeline on the chain's
    own bits for every row of every coded kind: verdict, both times, type-1 bits and rank -- no row left out on either side --, with T = 4
    (the default) and, on the hard route, T = 8 set through the handle.  The same handle without the flag equals the pipeline without
    rescue.  Rows are rescued, an SB1 among them, and a block behind a rescued SB1 differs from the run without the flag; with FLAG_BITERR
    every row's count is the definition's on the bits the row ends up with."""
    R = pkg.rx_binding
    base = {"hard": 0, "one_stream": R.FLAG_ONE_STREAM, "soft": R.FLAG_SOFT, "soft_biterr": R.FLAG_SOFT | R.FLAG_BITERR}[route]
    soft = oracle_stream[1] if base & R.FLAG_SOFT else None
    plain, plain_aach, plain_bits, _ = run_chain(pkg, iq, base)
    for T in ((None, 8) if route == "hard" else (None,)):
        rows, aach, bits, _ = run_chain(pkg, iq, base | R.FLAG_LIST, T)
        assert all(np.array_equal(a, b) for a, b in zip(bits, plain_bits))
        want = expected(oracle, bits, 4 if T is None else T, soft)
        want0 = expected(oracle, bits, 0, soft)
        assert set(rows) == set(want) == set(plain)
        for k in want:
            assert rows[k][:5] == want[k][:5], (route, T, k, rows[k][:3], want[k][:3], rows[k][4], want[k][4])
            assert plain[k][:4] == want0[k][:4], (route, k)
            if base & R.FLAG_BITERR:
                assert rows[k][5] == want[k][5] and plain[k][5] == want0[k][5], (route, k)
        rescued = [k for k in rows if rows[k][4] > 0]
        assert len(rescued) >= 3 and any(k[0] == ch.KIND_SB1 for k in rescued)
        assert all(rows[k][0] >= plain[k][0] for k in rows)
        assert LP.rescued_sb1_matters(rows, plain)
        if base & R.FLAG_BITERR:
            assert any(rows[k][5] != plain[k][5] for k in rescued)
        # the AACH has no rescue: the same rows (their bits follow the code a rescued SB1 may have supplied)
        assert len(aach) == len(plain_aach) and len(aach[0][0]) == len(plain_aach[0][0])


@pytest.mark.gpu
def test_gpu_chain_without_the_flag_refuses_and_bad_arguments(pkg):
    R = pkg.rx_binding
    assert R.FLAG_LIST == 512
    rx = pkg.RxChain(2, 4000)
    try:
        for f in (lambda: rx.fetch_list_rank(R.KIND_SCH_F), lambda: rx.set_list_candidates(4), lambda: rx.list_rank_device(R.KIND_SCH_F)):
            with pytest.raises(pkg.TetraDemodError) as e:
                f()
            assert e.value.status == ERR_UNSUPPORTED
    finally:
        rx.close()
    for bad in (4, 16, 64, 256):                               # still no flags
        with pytest.raises(pkg.TetraDemodError):
            pkg.RxChain(2, 4000, flags=R.FLAG_LIST | bad)
    rx = pkg.RxChain(2, 4000, flags=R.FLAG_LIST | R.FLAG_BITERR | R.FLAG_SYNC_TOLERANT | R.FLAG_AACH_RM3014, kinds=1 << R.KIND_SCH_F)
    try:
        for k in (R.KIND_BBK, R.KIND_SB2):                 # the AACH has no rank; SB2 is not decoded by this handle
            with pytest.raises(pkg.TetraDemodError) as e:
                rx.fetch_list_rank(k)
            assert e.value.status == ERR_UNSUPPORTED
        assert len(rx.fetch_list_rank(R.KIND_SCH_F)) == 0 and len(rx.fetch_list_rank(R.KIND_SB1)) == 0
        for T in (0, 9):
            with pytest.raises(pkg.TetraDemodError) as e:
                rx.set_list_candidates(T)
            assert e.value.status == ERR_ARG
        rx.set_list_candidates(1)
        rx.set_list_candidates(8)
    finally:
        rx.close()


@pytest.mark.gpu
def test_gpu_wideband_fetches_ranks(pkg, synth):
    """The wideband handle with the flag in cfg.rx.flags (the smallest configuration of tests/test_wbrx.py): its chain hands out a rank per
    coded row, and a rank says what the row's verdict is."""
    import torch
    from tests.test_wbrx import BINS_SMALL, CARRIERS_SMALL, D_SMALL, M_SMALL, _capture
    R = pkg.rx_binding
    x, _, _ = _capture(torch, synth, M_SMALL, CARRIERS_SMALL, 24)
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=x.shape[0], flags=R.FLAG_LIST)
    try:
        wb.rx.set_list_candidates(8)
        wb.process_device(x, x.shape[0], torch.cuda.current_stream())
        rows = 0
        for k in LP.CODED_KINDS:
            blocks, _ = wb.rx.fetch(k)
            rank = wb.rx.fetch_list_rank(k)
            assert len(rank) == len(blocks) and np.array_equal(rank >= 0, blocks["crc_ok"] != 0) and rank.min(initial=0) >= -1 and rank.max(initial=0) <= 8
            rows += len(rank)
        assert rows > 20
        with pytest.raises(pkg.TetraDemodError) as e:
            wb.rx.fetch_list_rank(R.KIND_BBK)
        assert e.value.status == ERR_UNSUPPORTED
    finally:
        wb.close()


@pytest.mark.gpu
def test_gpu_host_banks_fetch_ranks(pkg, synth, tmp_path):
    """TetraRxBank::setListCandidates / fetchListRank and the TetraRxMultiBank concatenation (host/tetra_rx_bank.h), 3 shards on one GPU
    against one bank of all channels and a bank without the flag: a plain C++ driver (tests/host/test_list_bank.cpp)."""
    import os
    import subprocess
    from tests.chain_host import noisy_batch as _noisy_batch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pk = os.path.join(root, "sdrpp-tetra-demodulator_amd")
    pkg.build.build()
    exe = os.path.join(root, "tests", "host", "test_list_bank")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(pk, "host"),
                    os.path.join(root, "tests", "host", "test_list_bank.cpp"), "-L", pk, "-ltetra_demod_hip", "-Wl,-rpath," + pk, "-o", exe], check=True)
    Cn, calls, nslots = 7, 2, 32
    N = nslots * 510 // calls
    _, _, iq = _noisy_batch(synth, Cn, nslots, N * calls, 8950)
    f = tmp_path / "iq.bin"
    with open(f, "wb") as fh:
        for k in range(calls):
            fh.write(np.ascontiguousarray(iq[:, k * N:(k + 1) * N]).astype(np.complex64).tobytes())
    r = subprocess.run([exe, str(Cn), str(N), str(calls), str(f), "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_list_bank: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[3]) > 100
