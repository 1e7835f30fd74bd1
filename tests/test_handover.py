"""Retune with a donor (include/ext/tetra_handover.h): a restarted channel inherits frame timing, cell and TDMA clock from another.

CPU: the lane code on the host (tests/emul/handover_emul.cpp: bsync_core.hpp's ASSIST state under both lock rules, handover_core.hpp's
planting and apply step) on planted bit streams, against literal statements of the rule, the reference's own tetra_tdma_time_add_tn and
the reference rule's restatement (oracle/burst_sync_oracle.c).  GPU: the chain against that emulation fed the chain's own demodulated
bits, and a wideband handle on a synthetic band of one base station (two carriers with the same cell and frame timing, the traffic
carrier with ONE SYNC burst per multiframe as on air) against a witness slot and against the plain retune."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.restart_gpu import (BIN_A, BIN_B, BIN_B2, BIN_C, BIN_EMPTY, B_SYNC_SLOTS, CALL, CUTS, DONOR_CELL, D_BAND, M_BAND, NORM_1, NORM_2, SYNC,
                               TS, assert_exported_and_bound, band_calls, band_capture, blocks_by_time as _blocks_by_time, build_and_run_bank_driver,
                               burst as _burst, chain_snap as _chain_snap, count_seqs as _count_seqs, downlink_bits as _downlink_bits, drive,
                               filler as _filler, has_gpu as _has_gpu, in_flight_and_waited, reference_clock, slot_index as _slot_index)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "handover_tdma.json")
ERR_ARG, ERR_UNSUPPORTED, ERR_NO_DEVICE = -1, -2, -3


@pytest.fixture(scope="module")
def em():
    from tests.emul import handover_emul_bind
    handover_emul_bind.build()
    return handover_emul_bind


def _bank_with_donor(em, bits_in_buf=137, F=51000, tol=None, use_batch=True, cell=DONOR_CELL, state=None):
    """Channel 0 a LOCKED donor (no bits fed: its state and cell are written as a tail would have left them), channel 1 the heir."""
    bank = em.Bank(2, tol=tol, use_batch=use_batch)
    bank.st[0] = (em.ST_LOCKED if state is None else state, bits_in_buf, F, F + TS)
    bank.cell[0] = cell
    bank.st[1], bank.cell[1], bank.carry[1], bank.assist[1] = 0x7A7A7A7A, 0x7A7A7A7A, 0x7A, 0x7A7A7A7A          # poisoned: the reset comes first
    return bank


def _rule_expect(f_minus_b, w):
    m = 0
    while f_minus_b + TS * m - w < 0:
        m += 1
    return f_minus_b + TS * m, m


# ---------------------------------------------------------------------------------------------------------------------- CPU


TDMA_STARTS = [(4, 5, 7), (4, 18, 7), (3, 18, 7), (4, 18, 60), (4, 18, 59), (1, 1, 1), (0, 0, 0), (2, 17, 60), (4, 17, 33)]
TDMA_KS = list(range(0, 10))


def test_planting_arithmetic_equals_the_rule_and_the_reference_clock(em):
    """expect and m for F - B in {0, -1, -509, -510, -1019} x W in {0, 1, 32, 127} against the rule written out; the heir's State, Assist
    and cell after the planting; its PHY time = the donor's advanced by m slots across the wraps tn 4 -> 1, fn 18 -> 1, mn 60 -> 1,
    against the reference's tetra_tdma_time_add_tn."""
    ref_clock = reference_clock([(start, k) for start in TDMA_STARTS for k in TDMA_KS], GOLDEN)
    for start in TDMA_STARTS:
        for k in TDMA_KS:
            assert em.tdma_steps(start, k) == ref_clock[start + (k,)], (start, k)
    assert ref_clock[(4, 5, 7, 1)] == (1, 6, 7) and ref_clock[(4, 18, 7, 1)] == (1, 1, 8) and ref_clock[(4, 18, 60, 1)] == (1, 1, 1)
    for fb in (0, -1, -509, -510, -1019):
        for w in (0, 1, 32, 127):
            want, m = _rule_expect(fb, w)
            assert em.expect(-fb, w) == (want, m), (fb, w)
            assert want - w >= 0 and (m == 0 or want - TS - w < 0)
            for phy in ((4, 18, 60), (3, 18, 7), (2, 9, 3)):
                cell = DONOR_CELL[:7] + phy
                bank = _bank_with_donor(em, bits_in_buf=-fb, cell=cell)
                bank.plant(1, 0, w, 72)
                assert bank.state(1) == (em.ST_ASSIST, 0, 0, 0)
                assert tuple(bank.assist[1]) == (em.PENDING, 0, 0, want, w, 72, 0, 0)
                assert tuple(bank.cell[1][:7]) == cell[:7] and tuple(bank.cell[1][7:]) == ref_clock.get(phy + (m,), em.tdma_steps(phy, m))
                assert not bank.carry[1].any()
                assert bank.state(0) == (em.ST_LOCKED, -fb, 51000, 51000 + TS) and tuple(bank.cell[0]) == cell          # the donor is only read


@pytest.mark.parametrize("tol", [None, (3, 5, 16)])
@pytest.mark.parametrize("W", [0, 1, 8, 32, 127])
def test_window_locks_inside_and_nowhere_else(em, synth, W, tol):
    """A normal burst planted so that its frame starts at expect + d: for |d| <= W the heir locks exactly there -- first frame at bit
    number expect + d with the burst's bits and type, state LOCKED with the frame consumed, status (LOCKED, 0, d), result word 1 -- and
    for d = +-(W + 1) it does not: still ASSIST one slot period on, nothing reported."""
    rng = np.random.default_rng(100 + W)
    ds = sorted({0, 1, -1, W, -W} & set(range(-W, W + 1)))
    for d in ds + [W + 1, -(W + 1)]:
        bank = _bank_with_donor(em, bits_in_buf=137, tol=tol)
        bank.plant(1, 0, W, 72)
        expect = bank.field(1, "expect")
        assert expect == _rule_expect(-137, W)[0]
        kind = (NORM_1, NORM_2)[d & 1]
        burst = _burst(synth, rng, kind)
        s = expect + d
        stream = np.concatenate([_filler(synth, rng, s), burst, _filler(synth, rng, W + 1 - d if abs(d) > W else 300)])
        assert _count_seqs(synth, stream) == [s + 244]
        # not a bit before the channel has received expect + W + 510 bits
        fr, ty, bn = bank.feed(1, stream[:expect + W + TS - 1])
        assert len(ty) == 0 and bank.state(1)[0] == em.ST_ASSIST and bank.status(1) == (em.PENDING, 0, 0)
        fr, ty, bn = bank.feed(1, stream[expect + W + TS - 1:expect + W + TS])
        if abs(d) <= W:
            assert list(ty) == [kind] and list(bn) == [s] and np.array_equal(fr[0], burst), d
            assert bank.state(1) == (em.ST_LOCKED, W - d, s + TS, s + 2 * TS), d
            assert bank.status(1) == (em.LOCKED, 0, d) and bank.field(1, "result") == 1
        else:
            assert len(ty) == 0 and bank.state(1)[0] == em.ST_ASSIST, d
            assert bank.status(1) == (em.PENDING, 1, 0) and bank.field(1, "result") == 0
            assert bank.field(1, "expect") == expect + TS and bank.field(1, "slots_left") == 71
            assert bank.state(1)[2] == expect + TS - W          # the bits before expect - W are dropped


@pytest.mark.parametrize("tol", [None, (3, 5, 16)])
def test_window_order_is_nearest_first_plus_before_minus_and_sync_bursts_lock(em, synth, tol):
    """Two planted matches, a sync sequence for a frame start at expect - 3 and normal sequence 1 for one at expect + 3 (their two shared
    bits agree): + 3 wins.  A sync burst alone locks at offset 214.  And a lock after k missed slot periods writes 1 + k, which the
    apply step turns into k slots on the heir's PHY time and nothing else."""
    rng = np.random.default_rng(7)
    W = 8
    bank = _bank_with_donor(em, tol=tol)
    bank.plant(1, 0, W, 72)
    expect = bank.field(1, "expect")
    stream = _filler(synth, rng, expect + W + TS + 40)
    stream[expect - 3 + 214:expect - 3 + 214 + 38] = synth.TRAIN_SYNC
    stream[expect + 3 + 244:expect + 3 + 244 + 22] = synth.TRAIN_NORM_1
    assert _count_seqs(synth, stream) == [expect - 3 + 214, expect + 3 + 244]
    fr, ty, bn = bank.feed(1, stream)
    assert bank.status(1) == (em.LOCKED, 0, 3) and list(bn[:1]) == [expect + 3] and ty[0] in (NORM_1, -1)
    # a sync burst, two slot periods late
    bank = _bank_with_donor(em, tol=tol)
    bank.plant(1, 0, W, 72)
    cell0 = tuple(bank.cell[1])
    s = expect + 2 * TS - 5
    burst = _burst(synth, rng, SYNC)
    stream = np.concatenate([_filler(synth, rng, s), burst, _filler(synth, rng, 100)])
    assert _count_seqs(synth, stream) == [s + 214]
    fr, ty, bn = bank.feed(1, stream)
    assert list(ty) == [SYNC] and list(bn) == [s] and np.array_equal(fr[0], burst)
    assert bank.status(1) == (em.LOCKED, 2, -5) and bank.field(1, "result") == 3
    bank.apply()
    assert bank.field(1, "result") == 0 and bank.status(1) == (em.LOCKED, 2, -5)
    assert tuple(bank.cell[1][:7]) == cell0[:7] and tuple(bank.cell[1][7:]) == em.tdma_steps(cell0[7:], 2)
    before = bank.cell.copy()
    bank.apply()                                       # consumed: a second apply changes nothing
    assert np.array_equal(bank.cell, before)


@pytest.mark.parametrize("tol", [None, (3, 5, 16)])
@pytest.mark.parametrize("W,max_slots", [(8, 3), (127, 1), (0, 5)])
def test_expiry_falls_back_to_the_reference_rule_on_what_is_buffered(em, synth, oracle, W, max_slots, tol):
    """No training sequence for max_slots slot periods: UNLOCKED, result word -1, status (EXPIRED, max_slots, 0), and the apply step
    zeroes the cell.  From there the frames are those of the reference's rule (oracle/burst_sync_oracle.c, one bit per call) fed the bits
    from the buffer's start on -- bit numbers counted from the heir's bit 0."""
    rng = np.random.default_rng(31 * W + max_slots)
    bank = _bank_with_donor(em, bits_in_buf=300, tol=tol)
    bank.plant(1, 0, W, max_slots)
    expect = bank.field(1, "expect")
    last = expect + TS * (max_slots - 1)                          # the last window's centre
    quiet = last + W + TS
    stream = np.concatenate([_filler(synth, rng, quiet), rng.integers(0, 2, 77, dtype=np.uint8), _downlink_bits(synth, rng, 14)])
    fr, ty, bn = bank.feed(1, stream[:quiet])
    start = last + TS - W
    assert len(ty) == 0 and bank.state(1) == (em.ST_UNLOCKED, quiet - start, start, 0)
    assert bank.status(1) == (em.EXPIRED, max_slots, 0) and bank.field(1, "result") == -1 and bank.cell[1].any()
    bank.apply()
    assert not bank.cell[1].any() and bank.field(1, "result") == 0 and bank.status(1) == (em.EXPIRED, max_slots, 0)
    fr, ty, bn = bank.feed(1, stream[quiet:])
    want = oracle.BurstSyncOracle()
    wfr, wty, wbn = want.feed(stream[start:])
    if tol is None:
        assert np.array_equal(ty, wty) and np.array_equal(bn, wbn + start) and np.array_equal(fr, wfr) and len(ty) >= 8
        ws = want.state
        assert bank.state(1) == (ws[0], ws[1], ws[2] + start, ws[3] + start)
    else:      # the tolerant rule's UNLOCKED and KNOW_FSTART are the reference's: the same first frame, and on this clean stream the same frames
        assert len(ty) >= 8 and np.array_equal(bn, wbn + start) and np.array_equal(fr, wfr)


@pytest.mark.parametrize("tol", [None, (3, 5, 16)])
@pytest.mark.parametrize("case", ["lock_late", "expire", "lock_at_edge"])
def test_cut_independence(em, synth, case, tol):
    """The same stream in cuts of 1, 509, 510, 511, 1020 bits and ragged sizes, with and without the LOCKED batch: frames, types, bit
    numbers, the result words in their order, the final State, Assist fields, cell and bit buffer are those of one single call."""
    rng = np.random.default_rng({"lock_late": 1, "expire": 2, "lock_at_edge": 3}[case])
    W, max_slots = (8, 4)
    probe = _bank_with_donor(em, tol=tol)
    probe.plant(1, 0, W, max_slots)
    expect = probe.field(1, "expect")
    if case == "expire":
        stream = np.concatenate([_filler(synth, rng, expect + TS * max_slots + 33), _downlink_bits(synth, rng, 9)])
    else:
        s = expect + 2 * TS + 3 if case == "lock_late" else expect + W
        stream = np.concatenate([_filler(synth, rng, s), _downlink_bits(synth, rng, 9), _filler(synth, rng, 700), _downlink_bits(synth, rng, 8)])

    def run(cut, use_batch):
        bank = _bank_with_donor(em, tol=tol, use_batch=use_batch)
        bank.plant(1, 0, W, max_slots)
        return bank.feed_in_cuts(1, stream, cut)

    whole = run(stream.size, True)
    assert len(whole[1]) >= (5 if case == "expire" else 16)          # (an UNLOCKED receiver needs 1020 bits and a sync burst first)
    assert whole[3] == [{"lock_late": 3, "expire": -1, "lock_at_edge": 1}[case]]
    for cut in CUTS:
        for use_batch in (True, False):
            assert run(cut, use_batch) == whole, (cut, use_batch)


def test_refused_donors_leave_a_plainly_reset_heir(em):
    """A donor that is UNLOCKED, one that is KNOW_FSTART and one that is LOCKED with scramb_init 0: the heir equals a plainly reset
    channel field for field -- State, bit buffer, cell --, with the status REFUSED and no other hand-over field set."""
    for state, cell in ((em.ST_UNLOCKED, DONOR_CELL), (em.ST_KNOW_FSTART, DONOR_CELL), (em.ST_LOCKED, (0,) + DONOR_CELL[1:])):
        bank = _bank_with_donor(em, state=state, cell=cell)
        plain = _bank_with_donor(em, state=state, cell=cell)
        bank.plant(1, 0, 8, 72)
        plain.reset(1)
        assert np.array_equal(bank.st, plain.st) and np.array_equal(bank.carry, plain.carry) and np.array_equal(bank.cell, plain.cell)
        assert tuple(bank.assist[1]) == (em.REFUSED, 0, 0, 0, 0, 0, 0, 0) and bank.status(1) == (em.REFUSED, 0, 0)
        assert bank.state(1) == (em.ST_UNLOCKED, 0, 0, 0) and not bank.cell[1].any()
        bank.apply()
        assert np.array_equal(bank.cell, plain.cell)


def test_handover_header_symbols_all_exported_and_bound(pkg):
    src = assert_exported_and_bound(pkg, os.path.join("ext", "tetra_handover.h"), pkg.rx_binding.RX_HANDOVER_EXPORTS + pkg.wbrx_binding.WBRX_HANDOVER_EXPORTS,
                                    (("tetra_wbrx.h", "tetra_wbrx_", 14), ("tetra_rx.h", "tetra_rx_", len(pkg.rx_binding.RX_EXPORTS)),
                                     ("tetra_retune.h", "tetra_", 3)))          # the pinned headers did not grow
    assert callable(pkg.RxChain.handover_channels) and callable(pkg.RxChain.handover_status) and callable(pkg.WidebandRx.handover_status)
    assert "donors" in pkg.WidebandRx.retune.__code__.co_varnames
    R = pkg.rx_binding
    assert (R.HANDOVER_DEFAULT_WINDOW, R.HANDOVER_DEFAULT_MAX_SLOTS) == tuple(int(re.search(r"#define TETRA_HANDOVER_DEFAULT_%s (\d+)" % k, src).group(1))
                                                                               for k in ("WINDOW", "MAX_SLOTS"))
    assert C.sizeof(R.HandoverParams) == 8 and C.sizeof(R.HandoverStatus) == 12


def test_handover_entry_points_without_a_gpu_return_no_device(pkg):
    """Every entry point of the header says TETRA_ERR_NO_DEVICE on a machine without a GPU, whatever it is given; with a GPU a NULL
    handle is an argument error."""
    pkg.rx_binding._lib()
    L = pkg.wbrx_binding._lib()
    four = (C.c_int32 * 4)(1, 2, 3, 4)
    prm = pkg.rx_binding.HandoverParams(8, 72)
    st = (pkg.rx_binding.HandoverStatus * 2)()
    want = ERR_ARG if _has_gpu() else ERR_NO_DEVICE
    assert L.tetra_rx_handover_channels_device(None, four, four, 4, C.byref(prm), None) == want
    assert L.tetra_rx_handover_channels_device(None, None, None, 0, None, None) == want
    assert L.tetra_wbrx_retune_from(None, four, four, C.byref(prm), None) == want
    assert L.tetra_wbrx_retune_from(None, None, None, None, None) == want
    assert L.tetra_rx_get_handover(None, 0, 2, st) == want


# ---------------------------------------------------------------------------------------------------------------------- GPU


def _coded_iq(synth, n_slots, seed, cell, esn0_db=25.0, tau=0.6, cfo=0.01, payload_seed=None):
    """A coded downlink of `cell` as one channel's IQ at a sample per bit; carriers of one base station share tau and cfo."""
    tx, _ = synth.gen_downlink(n_slots, seed if payload_seed is None else payload_seed, cell=cell)
    iq, _, _ = synth.gen_channel(n_slots * TS, seed + 100, bits=tx, amp=0.5, cfo=cfo, tau=tau, phase0=0.3 * seed, esn0_db=esn0_db)
    return iq


@pytest.mark.gpu
@pytest.mark.parametrize("slots2,tolerant", [(8, False), (70, False), (70, True)])
def test_gpu_chain_handover_equals_the_host_emulation(pkg, synth, em, slots2, tolerant):
    """Three channels of a plain chain -- a donor, an heir on a second carrier of the donor's cell and frame timing, a bystander on
    another cell -- in two calls (16 slots, then 8 or, across the tracker's 64-slot groups and the synchroniser's LOCKED batch, 70), the
    heir handed over between them.  The host emulation (tests/emul/handover_emul.cpp) is fed the chain's own demodulated bits call for
    call, with the planting and the apply step where the chain has them: State and hand-over status of all three channels, and the
    heir's reported frames (bit numbers; burst types through the kinds its rows come from) equal the emulation's.  The heir has
    locked inside the window, its first block's time is the donor's T advanced by m + k + 1 slots, and its blocks pass their CRC under
    the inherited scrambling code.  Donor and bystander equal a chain that saw no hand-over, byte for byte."""
    import torch
    from tests.chain_gpu import bit_rows as _bit_rows
    R = pkg.rx_binding
    slots1, cell = 16, (262, 1, 5)
    n = slots1 + slots2
    iq = np.stack([_coded_iq(synth, n, 1, cell), _coded_iq(synth, n, 1, cell, payload_seed=2), _coded_iq(synth, n, 3, (300, 7, 9), tau=1.3, cfo=-0.02)])
    flags = R.FLAG_SYNC_TOLERANT if tolerant else 0
    X, Z = (pkg.RxChain(3, slots2 * TS if slots2 > slots1 else slots1 * TS, flags=flags) for _ in range(2))
    bank = em.Bank(3, tol=(3, 5, 16) if tolerant else None)
    cut = slots1 * TS
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, :cut]))
    for c, b in enumerate(_bit_rows(torch, X, 3)):
        bank.feed(c, np.frombuffer(b, np.uint8))
    assert X.sync_states() == [bank.state(c) for c in range(3)]
    cells = X.cells()
    assert X.sync_states()[0][0] == em.ST_LOCKED and cells[0].scramb_init == synth.tx_scramb_code(*cell)          # (a donor that can give)
    assert X.handover_status() == [(em.NONE, 0, 0)] * 3
    for c in range(3):
        bank.cell[c] = [getattr(cells[c], f) for f in em.CELL_FIELDS]
    X.handover_channels([1], [0])
    bank.plant(1, 0, R.HANDOVER_DEFAULT_WINDOW, R.HANDOVER_DEFAULT_MAX_SLOTS)
    assert X.handover_status() == [bank.status(c) for c in range(3)] and X.handover_status()[1] == (em.PENDING, 0, 0)
    assert X.sync_states() == [bank.state(c) for c in range(3)] and X.sync_states()[1] == (em.ST_ASSIST, 0, 0, 0)
    planted = [getattr(X.cells()[1], f) for f in em.CELL_FIELDS]
    assert planted == [int(v) for v in bank.cell[1]]
    T, m = tuple(bank.cell[0][7:]), em.expect(bank.state(0)[1], R.HANDOVER_DEFAULT_WINDOW)[1]
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, cut:]))
    want = {}
    for c, b in enumerate(_bit_rows(torch, X, 3)):
        _, ty, bn = bank.feed(c, np.frombuffer(b, np.uint8))
        want[c] = {t: sorted(int(x) for x in bn[ty == t]) for t in (NORM_1, NORM_2, SYNC)}
    assert X.sync_states() == [bank.state(c) for c in range(3)]
    st = X.handover_status()
    assert st == [bank.status(c) for c in range(3)]
    assert st[1][0] == em.LOCKED and abs(st[1][2]) <= R.HANDOVER_DEFAULT_WINDOW and st[0] == st[2] == (em.NONE, 0, 0)
    rows = {k: X.fetch(k)[0] for k in range(R.N_KINDS)}
    for kind, t in ((R.KIND_SB1, SYNC), (R.KIND_SCH_F, NORM_1), (R.KIND_NDB1, NORM_2)):
        for c in range(3):
            assert sorted(int(b["bitnum"]) for b in rows[kind] if b["channel"] == c) == want[c][t], (kind, c)
    assert len(want[1][NORM_1]) + len(want[1][NORM_2]) >= slots2 // 2 - 2
    heir = sorted((int(b["bitnum"]), int(b["tdma_time_rx"]), int(b["crc_ok"])) for k in (R.KIND_SCH_F, R.KIND_NDB1, R.KIND_SB1) for b in rows[k] if b["channel"] == 1)
    tn, fn, mn = em.tdma_steps(T, m + st[1][1] + 1)
    assert heir[0][1] == tn | (fn << 8) | (mn << 16)
    coded = [b for k in (R.KIND_SCH_F, R.KIND_NDB1, R.KIND_NDB2, R.KIND_SB2) for b in rows[k] if b["channel"] == 1]
    assert coded and all(b["crc_ok"] == 1 for b in coded)
    donor_times = {(k, int(b["tdma_time_rx"])) for k in range(R.N_KINDS) for b in rows[k] if b["channel"] == 0}
    assert {(k, int(b["tdma_time_rx"])) for k in range(R.N_KINDS) for b in rows[k] if b["channel"] == 1} <= donor_times          # frame-synchronous carriers
    sx, sz = _chain_snap(pkg, X, 3), _chain_snap(pkg, Z, 3)
    assert sx[0] == sz[0] and sx[2] == sz[2] and sx[1] != sz[1]
    X.close(), Z.close()


@pytest.mark.gpu
def test_gpu_handover_refuses_bad_arguments_and_changes_nothing(pkg, synth):
    """Every TETRA_ERR_ARG case of both entry points: nothing is enqueued, the status reads NONE, the bin list and the counts stay, and all
    later output equals that of a handle that never saw the calls.  A wideband handle's chain refuses the chain's entry point."""
    R = pkg.rx_binding
    L = R._lib()
    iq = np.stack([_coded_iq(synth, 12, s, (262, 1, 5)) for s in (1, 2, 3)])
    X, Z = (pkg.RxChain(3, 6 * TS) for _ in range(2))
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, :6 * TS]))
    arr = lambda v: (C.c_int32 * len(v))(*v)
    ok_prm = R.HandoverParams(8, 72)
    for ch, dn, prm in (([1], [3], ok_prm), ([1], [-2], ok_prm), ([1], [1], ok_prm), ([1, 2], [0, 1], ok_prm), ([1, 1], [0, 0], ok_prm), ([3], [0], ok_prm),
                        ([1], [0], R.HandoverParams(128, 72)), ([1], [0], R.HandoverParams(-1, 72)), ([1], [0], R.HandoverParams(8, 0)),
                        ([1], [0], R.HandoverParams(8, 256)), ([0, 1, 2, 0], [-1] * 4, ok_prm)):
        assert L.tetra_rx_handover_channels_device(X._h, arr(ch), arr(dn), len(ch), C.byref(prm), None) == ERR_ARG, (ch, dn, prm.window, prm.max_slots)
    assert L.tetra_rx_handover_channels_device(X._h, arr([1]), None, 1, None, None) == ERR_ARG
    assert L.tetra_rx_handover_channels_device(X._h, None, arr([0]), 1, None, None) == ERR_ARG
    assert L.tetra_rx_handover_channels_device(X._h, arr([1]), arr([0]), -1, None, None) == ERR_ARG
    with pytest.raises(ValueError):
        X.handover_channels([1], [0, 0])
    X.handover_channels([], [])
    assert X.handover_status() == [(0, 0, 0)] * 3
    st = (R.HandoverStatus * 4)()
    assert L.tetra_rx_get_handover(X._h, 0, 4, st) == ERR_ARG and L.tetra_rx_get_handover(X._h, -1, 1, st) == ERR_ARG
    assert L.tetra_rx_get_handover(X._h, 0, 1, None) == ERR_ARG
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, 6 * TS:]))
    assert _chain_snap(pkg, X, 3) == _chain_snap(pkg, Z, 3)
    X.close(), Z.close()
    wb = pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16)
    W = pkg.wbrx_binding._lib()
    for bins, dn, prm in (([1, 8, 20], [-1, 3, -1], ok_prm), ([1, 8, 20], [-1, -2, -1], ok_prm), ([1, 8, 21], [-1, 2, -1], ok_prm),
                          ([1, 8, 20], [-1, 1, -1], ok_prm), ([1, 8, 20], [-1, 0, -1], R.HandoverParams(8, 0)), ([1, 8, 8], [-1, 0, -1], ok_prm)):
        assert W.tetra_wbrx_retune_from(wb._h, arr(bins), arr(dn), C.byref(prm), None) == ERR_ARG, (bins, dn)
    assert W.tetra_wbrx_retune_from(wb._h, None, arr([0, 0, 0]), None, None) == ERR_ARG
    assert list(wb.bins()) == [1, 7, 20] and wb.retune_count() == (0, 0) and wb.handover_status() == [(0, 0, 0)] * 3
    wb.retune([1, 7, 20], donors=[5, 5, 5])          # nothing moves: the donors are ignored, nothing changes
    assert wb.retune_count() == (1, 0)
    assert L.tetra_rx_handover_channels_device(wb.rx._h, arr([1]), arr([0]), 1, None, None) == ERR_UNSUPPORTED
    with pytest.raises(TypeError):
        wb.rx.handover_channels([1], [0])
    wb.close()


# The band of one base station: tests/restart_gpu.py.


@pytest.fixture(scope="module")
def band(pkg, synth):
    import torch
    return band_capture(torch, synth)


def _band_run(pkg, torch, xs, bins0, move=None, donors=None, stream=None, flags=0, wait=False, params=None):
    """Feed the capture in 0.25 s calls, retune to `move` before call 1; -> (per call the per-slot snapshots, per call the hand-over
    status, the handle)."""
    wb = pkg.WidebandRx(bins0, n_channels=M_BAND, decimation=D_BAND, max_in=CALL, flags=flags)
    before = {} if move is None else {1: lambda w: w.retune(move, stream, donors=donors, **(params or {}))}
    snaps, status = drive(pkg, torch, wb, xs, band_calls(xs.shape[0]), before, stream, wait)
    return snaps, status, wb


@pytest.mark.gpu
def test_gpu_moved_slot_with_a_donor_delivers_before_the_next_sync_burst(pkg, synth, band):
    """Slot 0 on carrier A throughout (the donor), slot 2 on carrier B throughout (the witness), slot 1 on an empty bin and moved onto
    carrier B at the first call boundary, just behind B's SYNC burst; 0.25 s calls, 1.1 s after the move.
      1. slots 0 and 2 equal a run that never retuned, bit for bit, call for call;
      2. from its first delivered frame on slot 1's blocks equal the witness's blocks of the same frames, matched by TDMA time and kind --
         every kind's type-1 bits, crc_ok, tdma_time_rx, tdma_time --, and its cell state at the end equals the witness's;
      3. slot 1 delivers its first CRC-good NDB or SCH/F block before the next SYNC burst of carrier B (slot 88 of the synthesis: B_SYNC_SLOTS);
      4. the same move through the plain tetra_wbrx_retune delivers none before that burst.
    3 and 4 together fail without the hand-over."""
    import torch
    R = pkg.rx_binding
    xs = band
    bins0, moved = [BIN_A, BIN_EMPTY, BIN_B], [BIN_A, BIN_B2, BIN_B]
    never, _, h0 = _band_run(pkg, torch, xs, bins0)
    with_donor, status, h1 = _band_run(pkg, torch, xs, bins0, move=moved, donors=[-1, 0, -1])
    plain, _, h2 = _band_run(pkg, torch, xs, bins0, move=moved)
    for i, (a, b, c) in enumerate(zip(never, with_donor, plain)):
        for slot in (0, 2):
            assert b[slot] == a[slot] and c[slot] == a[slot], (i, slot)
    assert status[0] == [(0, 0, 0)] * 3 and status[-1][1][0] == 2 and abs(status[-1][1][2]) <= R.HANDOVER_DEFAULT_WINDOW, status
    next_sync = B_SYNC_SLOTS[2]
    wit, _ = _blocks_by_time(with_donor, 2)
    heir, heir_order = _blocks_by_time(with_donor, 1, first_call=1)
    assert len(heir_order) >= 150 and len(heir) == len(heir_order)
    for key, val in heir.items():
        assert wit.get(key) == val, (key, val[:2], wit.get(key, (None, None))[:2])
    assert with_donor[-1][1]["cell"] == with_donor[-1][2]["cell"]
    # 3 and 4 by position in the moved slot's own bit stream, which starts at 0 at the move (sample CALL of the capture, a bit per
    # 800 / 36 samples): B's next SYNC burst begins (next_sync * 510 - move) bits later, plus the chain's delay, which only helps 4
    traffic = (R.KIND_NDB1, R.KIND_NDB2, R.KIND_SCH_F)
    burst_at = next_sync * TS - CALL * 36000 // 800000
    good_bits = lambda snaps: sorted(r[1] for s in snaps[1:] for k in traffic for r in s[1]["rows"][k] if r[2])
    with_bits, plain_bits = good_bits(with_donor), good_bits(plain)
    first_slot = min(_slot_index(t) for k, t, ok, ta, bits in heir_order if k in traffic and ok)
    print("first CRC-good traffic block of the moved slot: bit %d (TDMA slot %d) with a donor, %s plain; B's next SYNC burst (slot %d) begins at bit %d"
          % (with_bits[0], first_slot, plain_bits[0] if plain_bits else "none in the capture", next_sync, burst_at))
    assert with_bits[0] < burst_at and first_slot < next_sync
    assert not [b for b in plain_bits if b < burst_at]
    for h in (h0, h1, h2):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("one_stream", [False, True])
def test_gpu_handover_with_calls_in_flight(pkg, synth, band, one_stream):
    """process, retune with a donor, process ... on a side stream with no wait anywhere (two calls in flight; the two-stream chain and
    TETRA_RX_FLAG_ONE_STREAM) leaves the latest and the previous call's results, frames, all state and the hand-over status equal to the
    same sequence with tetra_rx_wait before and after the retune."""
    import torch
    fl = pkg.rx_binding.FLAG_ONE_STREAM if one_stream else 0
    bins0, moved = [BIN_A, BIN_EMPTY, BIN_B], [BIN_A, BIN_B2, BIN_B]
    (_, _, fast), (slow_snaps, slow_status, slow) = in_flight_and_waited(
        pkg, torch, lambda stream, wait: _band_run(pkg, torch, band, bins0, move=moved, donors=[-1, 0, -1], stream=stream, flags=fl, wait=wait))
    assert fast.handover_status() == slow.handover_status() and fast.handover_status()[1][0] == 2
    assert slow_status[1][1][0] in (1, 2)
    fast.rx.wait()
    fast.close(), slow.close()


@pytest.mark.gpu
def test_gpu_a_donor_on_another_cell_costs_nothing_beyond_the_plain_retune(pkg, synth, band):
    """The donor slot is on carrier C: the same frame timing, another colour code, so the scrambling code the heir inherits is wrong.  The
    heir locks; its coded blocks fail their CRC until carrier B's SYNC PDU (slot 88) arrives; from that PDU on its blocks equal the
    witness's, and at the end so does its cell."""
    import torch
    R = pkg.rx_binding
    xs = band
    snaps, status, wb = _band_run(pkg, torch, xs, [BIN_C, BIN_EMPTY, BIN_B], move=[BIN_C, BIN_B2, BIN_B], donors=[-1, 0, -1])
    assert status[-1][1][0] == 2 and abs(status[-1][1][2]) <= R.HANDOVER_DEFAULT_WINDOW
    wit, _ = _blocks_by_time(snaps, 2)
    _, order = _blocks_by_time(snaps, 1, first_call=1)
    coded = (R.KIND_SB2, R.KIND_NDB1, R.KIND_NDB2, R.KIND_SCH_F)
    at = [i for i, (k, t, ok, ta, bits) in enumerate(order) if k == R.KIND_SB1 and ok]
    assert at, "carrier B's second SYNC burst was not decoded"
    # delivery order is by kind inside a call: split by the time the SYNC PDU sets
    sync_slot = _slot_index(order[at[0]][3])
    assert sync_slot == B_SYNC_SLOTS[2]
    before = [(k, t, ok) for k, t, ok, ta, bits in order if k in coded and _slot_index(ta) < sync_slot and not (k == R.KIND_SB2 and _slot_index(ta) == sync_slot)]
    assert len(before) >= 60 and not any(ok for k, t, ok in before)
    after = [(k, t, ok, ta, bits) for k, t, ok, ta, bits in order if _slot_index(ta) >= sync_slot and k != R.KIND_SB1]
    assert len(after) >= 8
    for k, t, ok, ta, bits in after:
        if k in coded and _slot_index(t) > sync_slot:
            assert ok and wit.get((k, t)) == (ok, ta, bits), (k, _slot_index(t))
    assert snaps[-1][1]["cell"] == snaps[-1][2]["cell"]
    wb.close()


@pytest.mark.gpu
def test_gpu_host_banks_hand_over_per_shard(pkg):
    """TetraRxBank::handOver / handoverStatus and the TetraRxMultiBank forwarding (host/tetra_rx_bank.h), 2 shards on one GPU: entries go
    to the shard that holds them in its own numbering, a donor outside its heir's shard is TETRA_ERR_ARG with nothing enqueued, the
    status comes back in the bank's channel order.  A plain C++ driver (tests/host/test_handover_bank.cpp)."""
    r = build_and_run_bank_driver(pkg, "test_handover_bank", [7, 2])
    assert r.returncode == 0 and "test_handover_bank: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
