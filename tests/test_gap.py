"""Stream gaps (include/ext/tetra_gap.h): channels restarted after missing samples keep frame timing, cell and TDMA clock.

CPU: the lane code on the host (tests/emul/gap_emul.cpp: handover_core.hpp's anchor and planting arithmetic; the restart in the kernel's
order and the ASSIST state through tests/emul/handover_emul.cpp) against the rule written out, the reference's own tetra_tdma_time_add_tn and
the hand-over's planting.  GPU: the chain against that emulation fed the chain's own demodulated bits, against a handle that saw the
uninterrupted IQ and against one that was fed the cut stream without being told; the wideband handle on tests/restart_gpu.py's band
against a fresh handle, the uninterrupted run and the run that was not told."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.restart_gpu import (BIN_A, BIN_B, BIN_C, BIN_EMPTY, B_SYNC_SLOTS, CALL, CUTS, DONOR_CELL, D_BAND, M_BAND, NORM_1, NORM_2, SYNC, TS,
                               assert_exported_and_bound, band_calls, band_capture, blocks_by_time as _blocks_by_time, build_and_run_bank_driver,
                               chain_snap as _chain_snap, count_seqs as _count_seqs, downlink_bits as _downlink_bits, drive, filler as _filler,
                               has_gpu as _has_gpu, in_flight_and_waited, reference_clock, rows_by_time, slot_index as _slot_index, snap as _snap,
                               traffic_downlink as _traffic_downlink)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gap_tdma.json")
HEADER = os.path.join(ROOT, "include", "ext", "tetra_gap.h")
ERR_ARG, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_SIZE, ERR_ALIGN = -1, -2, -3, -6, -7
PERIOD = 4 * 18 * 60


def _header_int(name):
    return int(re.search(r"#define %s (\d+)" % name, open(HEADER).read()).group(1))


GAP_WINDOW, GAP_MAX_SLOTS = _header_int("TETRA_GAP_DEFAULT_WINDOW"), _header_int("TETRA_GAP_DEFAULT_MAX_SLOTS")


@pytest.fixture(scope="module")
def em():
    from tests.emul import gap_emul_bind
    gap_emul_bind.build()
    return gap_emul_bind


# ---------------------------------------------------------------------------------------------------------------------- CPU

BITS_IN_BUF = (0, 1, 137, 509)
ELAPSED = (0, 1, 373, 509, 510, 511, 510 * 4320, 510 * 4320 + 77, 2 ** 31 - 1)
WINDOWS = (0, 8, 127)
PHYS = ((2, 9, 3), (4, 18, 60), (3, 18, 7))


def _rule(d, G, W):
    """m = the smallest integer >= 0 with 510 m - (d + G) >= W, and expect -- in Python's integers"""
    m = max(0, -(-(W + d + G) // TS))
    assert TS * m - (d + G) >= W and (m == 0 or TS * (m - 1) - (d + G) < W)
    return TS * m - (d + G), m


def _locked_bank(em, bits_in_buf, phy, n=1, F=51000, tol=None, use_batch=True):
    """Channel 0 LOCKED with bits_in_buf buffered bits, DONOR_CELL's code and the PHY time phy, as a tail would have left it; its bit
    buffer and miss counter hold what a running channel's hold (anything)."""
    bank = em.Bank(n, tol=tol, use_batch=use_batch)
    bank.st[0] = (em.ST_LOCKED, bits_in_buf, F, F + TS)
    bank.cell[0] = DONOR_CELL[:7] + tuple(phy)
    bank.carry[0], bank.miss[0] = 0x01, 3
    return bank


def _planting_cases():
    return sorted({(phy, _rule(b, G, W)[1] % PERIOD) for phy in PHYS for b in BITS_IN_BUF for G in ELAPSED for W in WINDOWS} | {(phy, PERIOD) for phy in PHYS})


def test_planting_arithmetic_equals_the_rule_and_the_reference_clock(em):
    """LOCKED anchors with bits_in_buf in {0, 1, 137, 509} x G in {0, 1, 373, 509, 510, 511, 510 * 4320, 510 * 4320 + 77, 2^31 - 1} x
    W in {0, 8, 127}: expect and m equal the rule written out, expect - W lies in [0, 510), the resumed channel's State, hand-over fields and
    cell are the rule's, its PHY time is the old one advanced by m steps of the reference's tetra_tdma_time_add_tn -- taken m mod 4320
    times, which the lane code's own clock taken m times agrees with, the reference's clock having the period 4320 --, and G = 0 equals the
    hand-over's planting from a donor with the same state."""
    assert em.tdma_period() == PERIOD
    ref_clock = reference_clock(_planting_cases(), GOLDEN)
    for phy in PHYS:
        assert ref_clock[phy + (PERIOD,)] == phy and em.tdma_steps(phy, PERIOD) == phy
    for b in BITS_IN_BUF:
        for G in ELAPSED:
            for W in WINDOWS:
                want, m = _rule(b, G, W)
                assert em.expect(b, G, W) == (want, m), (b, G, W)
                assert 0 <= want - W < TS
                for phy in PHYS:
                    bank = _locked_bank(em, b, phy)
                    assert bank.anchor(0) == (1, b, phy)
                    bank.resume(0, G, W, 72)
                    assert bank.state(0) == (em.ST_ASSIST, 0, 0, 0) and not bank.carry[0].any() and bank.miss[0] == 0
                    assert tuple(bank.assist[0]) == (em.PENDING, 0, 0, want, W, 72, 0, 0)
                    assert tuple(bank.cell[0][:7]) == DONOR_CELL[:7]
                    assert tuple(bank.cell[0][7:]) == ref_clock[phy + (m % PERIOD,)] == em.tdma_steps(phy, m), (b, G, W, phy)
    # G = 0: the hand-over's planting with the channel as its own donor
    for b in BITS_IN_BUF:
        for W in WINDOWS:
            for phy in PHYS:
                own, other = _locked_bank(em, b, phy), _locked_bank(em, b, phy, n=2)
                own.resume(0, 0, W, 72)
                other.plant(1, 0, W, 72)
                assert own.state(0) == other.state(1) and tuple(own.assist[0]) == tuple(other.assist[1]) and tuple(own.cell[0]) == tuple(other.cell[1])


def test_a_locked_channel_as_its_own_donor_equals_its_resume_after_no_gap(em):
    """Exhaustively, for bits_in_buf 0 .. 4096 x window 0 .. 127 x max_slots in {1, 72, 255}: a LOCKED channel restarted as the heir of
    itself taken as a donor (the hand-over's route: a source that must be LOCKED, no elapsed bits) and as its own heir after a gap of 0
    bits (the gap's route) ends with identical State, hand-over fields and cell, planted in every case.  The one restart of
    tetra_retune.hip rests on this identity; the loop runs in the emulation (tests/emul/handover_emul.cpp)."""
    for phy in PHYS:
        differing, planted, first = em.own_donor_vs_resume(DONOR_CELL[:7] + phy, 4096, 127, (1, 72, 255))
        assert (differing, planted) == (0, 4097 * 128 * 3), (phy, differing, planted, first)
    # (the comparison sees a difference where there is one: PENDING is accepted on one route only, a refused source leaves no planting)
    bank = em.Bank(1)
    bank.st[0], bank.cell[0], bank.assist[0] = (em.ST_ASSIST, 100, 0, 0), DONOR_CELL, (em.PENDING, 2, 0, 600, 8, 70, 0, 0)
    as_donor, as_own = em.Bank(1), em.Bank(1)
    for b, accept in ((as_donor, False), (as_own, True)):
        b.st[:], b.cell[:], b.assist[:] = bank.st, bank.cell, bank.assist
        b.restart(0, 0, accept, 0, 8, 72)
    assert as_donor.status(0) == (em.REFUSED, 0, 0) and as_own.status(0) == (em.PENDING, 0, 0)


@pytest.mark.parametrize("tol", [None, (3, 5, 16)])
@pytest.mark.parametrize("missed", [0, 1, 5])
@pytest.mark.parametrize("G", [0, 373, 3 * TS + 200])
def test_carry_over_from_assist(em, synth, missed, G, tol):
    """A channel planted by a hand-over and advanced by 0, 1 and 5 missed slot periods is resumed after G lost bits; the true frame start is
    where the rule says (on the planted grid, 3 bits late).  It locks on the same burst as the same channel left alone on the unbroken
    stream, with the same offset, and after the apply step both hold the same cell -- the same time for that frame and every later one."""
    rng = np.random.default_rng(1000 * missed + G)
    W = 8

    def planted():
        bank = em.Bank(2, tol=tol)
        bank.st[0] = (em.ST_LOCKED, 137, 51000, 51000 + TS)
        bank.cell[0] = DONOR_CELL
        bank.plant(1, 0, W, 72)
        return bank

    expect0 = planted().field(1, "expect")
    rcv = expect0 + TS * missed + W + 100          # the window of slot period `missed` has not been tried yet
    J = missed + (rcv - expect0 - TS * missed + G + W) // TS + 2
    P = expect0 + TS * J + 3
    stream = np.concatenate([_filler(synth, rng, P), _downlink_bits(synth, rng, 9)])
    assert _count_seqs(synth, stream)[0] >= P + 214 and P - 3 - W >= rcv + G

    def run(gap):
        bank = planted()
        bank.feed(1, stream[:rcv])
        bank.apply()
        assert bank.status(1) == (em.PENDING, missed, 0) and bank.field(1, "expect") == expect0 + TS * missed
        at = rcv
        if gap:
            q = em.tdma_steps(tuple(bank.cell[1][7:]), missed)
            assert bank.anchor(1) == (1, rcv - (expect0 + TS * missed), q)
            bank.resume(1, G, W, 72)
            want, m = _rule(rcv - (expect0 + TS * missed), G, W)
            assert tuple(bank.assist[1]) == (em.PENDING, 0, 0, want, W, 72, 0, 0) and tuple(bank.cell[1][7:]) == em.tdma_steps(q, m)
            assert rcv + G + want == expect0 + TS * (missed + m)          # the planted grid, in the new numbering
            at = rcv + G
        fr, ty, bn = bank.feed(1, stream[at:])
        assert bank.field(1, "result") == 1 + bank.field(1, "waited")
        bank.apply()
        return [f.tobytes() for f in fr], list(ty), [int(x) + (at if gap else 0) for x in bn], bank.status(1), tuple(bank.cell[1]), bank.state(1)[0]

    alone, resumed = run(False), run(True)
    assert alone[2][0] == P and alone[3] == (em.LOCKED, J, 3) and len(alone[1]) >= 8
    assert resumed[:3] == alone[:3] and resumed[3][0] == em.LOCKED and resumed[3][2] == 3
    assert resumed[4] == alone[4] and tuple(alone[4][7:]) == em.tdma_steps(DONOR_CELL[7:], em.expect(137, 0, W)[1] + J)
    assert resumed[5] == alone[5]


def test_refused_channels_are_plainly_reset(em):
    """UNLOCKED, KNOW_FSTART, LOCKED with scramb_init 0, and ASSIST whose status is not PENDING: the channel equals a plainly reset one
    field for field -- State, bit buffer, cell, miss counter --, status REFUSED and no other hand-over field set."""
    for state, cell, status in ((em.ST_UNLOCKED, DONOR_CELL, em.NONE), (em.ST_KNOW_FSTART, DONOR_CELL, em.NONE), (em.ST_LOCKED, (0,) + DONOR_CELL[1:], em.NONE),
                                (em.ST_ASSIST, DONOR_CELL, em.NONE), (em.ST_ASSIST, (0,) + DONOR_CELL[1:], em.PENDING)):
        def mk():
            bank = em.Bank(2)
            for c in (0, 1):
                bank.st[c] = (state, 137, 51000, 51000 + TS)
                bank.cell[c] = cell
                bank.carry[c], bank.miss[c] = 0x01, 5
                bank.assist[c] = (status, 2, 0, 51100, 8, 70, 0, 0)
            return bank
        bank, plain = mk(), mk()
        assert bank.anchor(0)[0] == 0
        bank.resume(0, 373, 8, 72)
        plain.reset(0)
        assert np.array_equal(bank.st, plain.st) and np.array_equal(bank.carry, plain.carry) and np.array_equal(bank.cell, plain.cell)
        assert np.array_equal(bank.miss, plain.miss) and np.array_equal(bank.assist[1], plain.assist[1])
        assert tuple(bank.assist[0]) == (em.REFUSED, 0, 0, 0, 0, 0, 0, 0) and bank.state(0) == (em.ST_UNLOCKED, 0, 0, 0) and not bank.cell[0].any()
        bank.apply()
        assert np.array_equal(bank.cell, plain.cell)


@pytest.mark.parametrize("tol", [None, (3, 5, 16)])
@pytest.mark.parametrize("case", ["lock_late", "expire", "lock_at_edge"])
def test_cut_independence_after_a_resume(em, synth, case, tol):
    """The stream behind a resume in tests/restart_gpu.py's cuts (1, 509, 510, 511, 1020 bits and ragged sizes), with and without the
    LOCKED batch, under both lock rules: frames, types, bit numbers, the result words in their order, the final State, hand-over fields,
    cell, bit buffer and miss counter are those of one single call."""
    rng = np.random.default_rng({"lock_late": 11, "expire": 12, "lock_at_edge": 13}[case])
    W, max_slots, G = 8, 4, 3 * TS + 200
    probe = _locked_bank(em, 137, (2, 9, 3), tol=tol)
    probe.resume(0, G, W, max_slots)
    expect = probe.field(0, "expect")
    assert expect == _rule(137, G, W)[0]
    if case == "expire":
        stream = np.concatenate([_filler(synth, rng, expect + TS * max_slots + 33), _downlink_bits(synth, rng, 9)])
    else:
        s = expect + 2 * TS + 3 if case == "lock_late" else expect + W
        stream = np.concatenate([_filler(synth, rng, s), _downlink_bits(synth, rng, 9), _filler(synth, rng, 700), _downlink_bits(synth, rng, 8)])

    def run(cut, use_batch):
        bank = _locked_bank(em, 137, (2, 9, 3), tol=tol, use_batch=use_batch)
        bank.resume(0, G, W, max_slots)
        return bank.feed_in_cuts(0, stream, cut)

    whole = run(stream.size, True)
    assert len(whole[1]) >= (5 if case == "expire" else 16)
    assert whole[3] == [{"lock_late": 3, "expire": -1, "lock_at_edge": 1}[case]]
    for cut in CUTS:
        for use_batch in (True, False):
            assert run(cut, use_batch) == whole, (cut, use_batch)


def test_gap_header_symbols_all_exported_and_bound(pkg):
    R, Wb = pkg.rx_binding, pkg.wbrx_binding
    names = R.RX_GAP_EXPORTS + Wb.WBRX_GAP_EXPORTS
    # (the pinned headers did not grow, and neither did RX_EXPORTS)
    assert_exported_and_bound(pkg, os.path.join("ext", "tetra_gap.h"), names, (("tetra_wbrx.h", "tetra_wbrx_", 14), ("tetra_rx.h", "tetra_rx_", len(R.RX_EXPORTS)),
                                                                              ("tetra_retune.h", "tetra_", 3), (os.path.join("ext", "tetra_handover.h"), "tetra_", 3)))
    assert callable(pkg.RxChain.resume) and callable(pkg.WidebandRx.gap) and callable(pkg.WidebandRx.process_device_at)
    assert (R.GAP_DEFAULT_WINDOW, R.GAP_DEFAULT_MAX_SLOTS, R.GAP_MAX_ELAPSED_BITS) == (GAP_WINDOW, GAP_MAX_SLOTS, _header_int("TETRA_GAP_MAX_ELAPSED_BITS"))
    assert R.GAP_MAX_ELAPSED_BITS == 2 ** 31 - 1 and GAP_WINDOW % 8 == 0 and GAP_WINDOW >= 8
    iq = open(os.path.join(ROOT, "include", "ext", "tetra_iqcond.h")).read()
    assert all(("#define TETRA_IQ_FMT_%s %d" % (n, v)) in iq for n, v in (("C64", Wb.IQ_FMT_C64), ("CS16", Wb.IQ_FMT_CS16), ("CS8", Wb.IQ_FMT_CS8)))
    assert len(R.RX_EXPORTS) == 16 and not set(names) & set(R.RX_EXPORTS + R.RX_HANDOVER_EXPORTS + Wb.WBRX_EXPORTS + Wb.WBRX_HANDOVER_EXPORTS)


def test_gap_entry_points_without_a_gpu_return_no_device(pkg):
    """Every entry point of the header says TETRA_ERR_NO_DEVICE on a machine without a GPU, whatever it is given; with a GPU a NULL
    handle is an argument error."""
    pkg.rx_binding._lib()
    L = pkg.wbrx_binding._lib()
    four = (C.c_int32 * 4)(0, 1, 2, 3)
    prm = pkg.rx_binding.HandoverParams(8, 72)
    g = C.c_int64(0)
    want = ERR_ARG if _has_gpu() else ERR_NO_DEVICE
    assert L.tetra_rx_resume_channels_device(None, four, 4, 137, C.byref(prm), None) == want
    assert L.tetra_rx_resume_channels_device(None, None, 0, -1, None, None) == want
    assert L.tetra_wbrx_gap(None, 1000, C.byref(prm), C.byref(g), None) == want
    assert L.tetra_wbrx_gap(None, -1, None, None, None) == want
    assert L.tetra_wbrx_process_device_at(None, None, 1, 0, 0, None, None) == want
    assert L.tetra_wbrx_process_device_at(None, four, 7, 4, -5, C.byref(prm), None) == want


# ---------------------------------------------------------------------------------------------------------------------- GPU: the chain

CELL_1, CELL_2 = (262, 1, 5), (300, 7, 9)
SLOTS_1, SLOTS_2 = 16, 24
TRAFFIC = (5, 3, 4)                                # KIND_SCH_F, KIND_NDB1, KIND_NDB2


def _sparse_iq(synth, n_slots, seed, cell, sync_slots, tau, cfo):
    """A coded downlink of `cell` with SYNC bursts only in sync_slots, as one channel's IQ at a sample per bit."""
    tx = _traffic_downlink(synth, n_slots, seed, cell, sync_slots)
    return synth.gen_channel(n_slots * TS, seed + 100, bits=tx, amp=0.5, cfo=cfo, tau=tau, phase0=0.3 * seed, esn0_db=25.0)[0]


def _three_channels(synth, removed, tolerant, seeds=(1, 3)):
    """Two carriers of different cells and noise, SLOTS_1 slots + `removed` samples + SLOTS_2 slots.  Each carrier has SYNC bursts in slots 4
    and 8 (a receiver locks on the first it sees and decodes the second), and late in the second call what a receiver that was not told
    about the gap needs to find its frame start again without decoding a SYNC PDU: under the reference's rule one SYNC burst to unlock on
    (misaligned, it stays LOCKED on normal bursts) and one to lock on, under the tolerant rule one behind its 16 missed frames.  The timing
    offset is one from which a freshly started timing loop settles before the first frame it reports, on both sides of the gap: the
    symbol grid on the sample grid for an even number of removed samples, a quarter of a symbol off it for an odd one, which moves the
    grid by half a symbol.  (Restarted half a symbol off, the demodulator needs fifteen slots and delivers bit errors meanwhile, which is
    the restart's doing and the same after a retune)"""
    after = SLOTS_1 + -(-removed // TS)
    n = after + SLOTS_2 + 1
    sync = (4, 8) + ((after + 18,) if tolerant else (after + 8, after + 12))
    rng = np.random.default_rng(5)
    noise = (0.1 * (rng.standard_normal(n * TS) + 1j * rng.standard_normal(n * TS))).astype(np.complex64)
    tau = 0.5 if removed % 2 else 0.0
    return np.stack([_sparse_iq(synth, n, seeds[0], CELL_1, sync, tau, 0.01), _sparse_iq(synth, n, seeds[1], CELL_2, sync, tau, -0.02), noise])


def _by_time(rows_by_kind):
    """{(channel, kind, tdma_time_rx): (crc_ok, tdma_time, type-1 bits)}; every key must be there once"""
    out, order = rows_by_time([rows_by_kind])
    assert len(out) == len(order)
    return out


def _by_bits(rows_by_kind, kinds=TRAFFIC):
    """{(channel, kind, type-1 bits): tdma_time_rx} of the CRC-good rows of the coded traffic kinds (random payloads: unique)"""
    return {(r[0], k, r[5]): r[3] for k in kinds for r in rows_by_kind[k] if r[2]}


@pytest.mark.gpu
@pytest.mark.parametrize("g,tolerant", [(137, False), (3 * TS + 200, False), (3 * TS + 200, True)])
def test_gpu_chain_resume_equals_the_host_emulation(pkg, synth, em, g, tolerant):
    """Three channels at a sample per bit, 16 slots, g samples removed from all three, resume(g), 24 slots.  The host emulation fed the
    chain's own demodulated bits call for call gives equal sync states, hand-over status, planted cells and reported frames; both carriers
    are LOCKED inside the default window, the noise channel is REFUSED.  Every block behind the gap equals, by (kind, tdma_time_rx), the
    block of a second handle that processed the uninterrupted IQ, in type-1 bits, crc_ok and tdma_time.  A third handle fed the same cut
    stream without the call delivers CRC-good blocks behind the gap whose times differ from the uninterrupted run's for the same bits.
    The last two together fail without the resume."""
    import torch
    from tests.chain_gpu import bit_rows, collect
    R = pkg.rx_binding
    iq = _three_channels(synth, g, tolerant, seeds=(1, 9) if g % 2 else (1, 3))
    cut, end = SLOTS_1 * TS, SLOTS_1 * TS + g + SLOTS_2 * TS
    flags = R.FLAG_SYNC_TOLERANT if tolerant else 0
    X, Z, U = (pkg.RxChain(3, 16000, flags=flags) for _ in range(3))          # resumed, uninterrupted, cut but untold
    bank = em.Bank(3, tol=(3, 5, 16) if tolerant else None)
    for h in (X, Z, U):
        h.process(np.ascontiguousarray(iq[:, :cut]))
    for c, b in enumerate(bit_rows(torch, X, 3)):
        bank.feed(c, np.frombuffer(b, np.uint8))
    cells = X.cells()
    assert X.sync_states() == [bank.state(c) for c in range(3)] and [s[0] for s in X.sync_states()] == [em.ST_LOCKED, em.ST_LOCKED, em.ST_UNLOCKED]
    assert [cells[c].scramb_init for c in range(3)] == [synth.tx_scramb_code(*CELL_1), synth.tx_scramb_code(*CELL_2), 0]
    assert X.handover_status() == [(em.NONE, 0, 0)] * 3
    for c in range(3):
        bank.cell[c] = [getattr(cells[c], f) for f in em.CELL_FIELDS]
    X.resume(g)
    for c in range(3):
        bank.resume(c, g, GAP_WINDOW, GAP_MAX_SLOTS)
    assert X.handover_status() == [bank.status(c) for c in range(3)] == [(em.PENDING, 0, 0), (em.PENDING, 0, 0), (em.REFUSED, 0, 0)]
    assert X.sync_states() == [bank.state(c) for c in range(3)] and X.sync_states()[2] == (em.ST_UNLOCKED, 0, 0, 0)
    assert [[getattr(cl, f) for f in em.CELL_FIELDS] for cl in X.cells()] == [[int(v) for v in bank.cell[c]] for c in range(3)]
    for h in (X, U):
        h.process(np.ascontiguousarray(iq[:, cut + g:end]))
    Z.process(np.ascontiguousarray(iq[:, cut:end]))
    want = {}
    for c, b in enumerate(bit_rows(torch, X, 3)):
        _, ty, bn = bank.feed(c, np.frombuffer(b, np.uint8))
        bank.apply()
        want[c] = {t: sorted(int(x) for x in bn[ty == t]) for t in (NORM_1, NORM_2, SYNC)}
    st = X.handover_status()
    print("g = %d, tolerant = %s: hand-over status %s" % (g, tolerant, st))
    assert X.sync_states() == [bank.state(c) for c in range(3)] and st == [bank.status(c) for c in range(3)]
    assert [[getattr(cl, f) for f in em.CELL_FIELDS][:4] for cl in X.cells()] == [[int(v) for v in bank.cell[c][:4]] for c in range(3)]
    assert st[0][0] == st[1][0] == em.LOCKED and abs(st[0][2]) <= GAP_WINDOW and abs(st[1][2]) <= GAP_WINDOW and st[2] == (em.REFUSED, 0, 0)
    rx, rz, ru = collect(X, R), collect(Z, R), collect(U, R)
    for kind, t in ((R.KIND_SB1, SYNC), (R.KIND_SCH_F, NORM_1), (R.KIND_NDB1, NORM_2)):
        for c in range(3):
            assert sorted(r[1] for r in rx[kind] if r[0] == c) == want[c][t], (kind, c)
    whole, got = _by_time(rz), _by_time(rx)
    wrong = [(k, v[:2], whole.get(k, (None, None))[:2]) for k, v in got.items() if whole.get(k) != v]
    by_bits = _by_bits(rz)
    # (the untold handle's first frame of the second call began in front of the gap: behind the gap is what the uninterrupted run times there)
    behind = SLOTS_1 + -(-g // TS)
    untold = [(k[:2], t, by_bits[k]) for k, t in _by_bits(ru).items() if k in by_bits and _slot_index(by_bits[k]) >= behind]
    print("blocks behind the gap: %d, of them unlike the uninterrupted run's %d; CRC-good blocks of the untold handle found in the uninterrupted run: %d, "
          "with its time %d" % (len(got), len(wrong), len(untold), sum(t == tz for _, t, tz in untold)))
    for c in (0, 1):
        assert sum(1 for k in got if k[0] == c and k[1] in TRAFFIC and got[k][0]) >= 12, c
    assert not [k for k in got if k[0] == 2]
    assert not wrong and untold and all(t != tz for _, t, tz in untold), (wrong[:4], untold[:4])
    sx, sz = _by_time({k: [r for r in v if r[0] == 2] for k, v in rx.items()}), _by_time({k: [r for r in v if r[0] == 2] for k, v in rz.items()})
    assert sx == sz == {}
    for h in (X, Z, U):
        h.close()


@pytest.mark.gpu
def test_gpu_two_gaps_the_second_while_pending(pkg, synth):
    """resume(600), a call of 300 bits -- too few for ASSIST to try its window --, resume(400) on channels that are PENDING, then 24 slots:
    both carriers lock inside the window, and every block behind the gaps equals the uninterrupted run's of the same kind and time."""
    from tests.chain_gpu import collect
    R = pkg.rx_binding
    g1, mid, g2 = 600, 300, 400
    iq = _three_channels(synth, g1 + mid + g2, False)
    cut = SLOTS_1 * TS
    end = cut + g1 + mid + g2 + SLOTS_2 * TS
    X, Z = (pkg.RxChain(3, 16000) for _ in range(2))
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, :cut]))
    X.resume(g1)
    X.process(np.ascontiguousarray(iq[:, cut + g1:cut + g1 + mid]))
    assert X.handover_status() == [(1, 0, 0), (1, 0, 0), (4, 0, 0)] and [s[0] for s in X.sync_states()] == [3, 3, 0] and X.sync_states()[0][1] > 0
    X.resume(g2)
    assert X.handover_status() == [(1, 0, 0), (1, 0, 0), (4, 0, 0)] and [s[:2] for s in X.sync_states()[:2]] == [(3, 0)] * 2
    X.process(np.ascontiguousarray(iq[:, cut + g1 + mid + g2:end]))
    Z.process(np.ascontiguousarray(iq[:, cut:end]))
    st = X.handover_status()
    print("two gaps: hand-over status", st)
    assert st[0][0] == st[1][0] == 2 and abs(st[0][2]) <= GAP_WINDOW and abs(st[1][2]) <= GAP_WINDOW and st[2] == (4, 0, 0)
    whole, got = _by_time(collect(Z, R)), _by_time(collect(X, R))
    assert sum(1 for k in got if k[1] in TRAFFIC and got[k][0]) >= 24
    assert not [(k, v[:2], whole.get(k, (None, None))[:2]) for k, v in got.items() if whole.get(k) != v]
    X.close(), Z.close()


@pytest.mark.gpu
def test_gpu_the_three_restarts_leave_what_the_host_emulation_leaves(pkg, synth, em):
    """One plain chain of 4 channels at a sample per bit under TETRA_RX_FLAG_SYNC_TOLERANT | TETRA_RX_FLAG_BITERR, so that the tail keeps
    all its tables: two carriers that fall silent for the last three of 16 slots (LOCKED, misses counted, link figures gathered) and two
    noise channels.  Four handles see the same call; then one gets reset_channels([1, 3]), one handover_channels([2, 3], [0, -1]), one
    resume(137, channels=[0, 2]), one nothing.  After each restart the listed channels' synchroniser state, cell, link figures, miss
    counter and hand-over status equal the host emulation's (tests/emul/restart_lanes.hpp) started from the handle's own tables, and the
    channels not listed equal the handle that was never restarted.  Last, the resumed handle hands channel 3 over from channel 0, which
    is PENDING now: a donor must be LOCKED, so the heir reads REFUSED.  A table that the single kernel forgot, or a planting from the
    wrong source, shows here."""
    import copy
    import torch
    from tests.chain_gpu import bit_rows
    R = pkg.rx_binding
    n, quiet = SLOTS_1 * TS, 3 * TS
    rng = np.random.default_rng(17)
    noise = lambda k: (0.1 * (rng.standard_normal(k) + 1j * rng.standard_normal(k))).astype(np.complex64)
    iq = np.concatenate([_three_channels(synth, 0, True)[:, :n], noise(n)[None, :]])
    iq[0, n - quiet:], iq[1, n - quiet:] = noise(quiet), noise(quiet)
    iq = np.ascontiguousarray(iq)
    plain, heirs, own, never = (pkg.RxChain(4, 16000, flags=R.FLAG_SYNC_TOLERANT | R.FLAG_BITERR) for _ in range(4))
    for h in (plain, heirs, own, never):
        h.process(iq)

    def link_words(h):
        return np.array([(v["bits"], v["bit_errors"], v["blocks"], v["blocks_crc_bad"]) for v in h.links()], R.LINK_DTYPE).view(np.uint32).reshape(4, -1)

    def tables(h):
        """per channel (sync state, cell, link figures as words, miss counter, hand-over status)"""
        cells, link, miss, status = h.cells(), link_words(h), h.sync_misses(), h.handover_status()
        return [(sync, [getattr(cells[c], f) for f in em.CELL_FIELDS], [int(v) for v in link[c]], int(miss[c]), status[c]) for c, sync in enumerate(h.sync_states())]

    def bank_tables(b):
        return [(b.state(c), [int(v) for v in b.cell[c]], [int(v) for v in b.link[c]], int(b.miss[c]), b.status(c)) for c in range(4)]

    bank = em.Bank(4, tol=(3, 5, 16))
    for c, b in enumerate(bit_rows(torch, never, 4)):
        bank.feed(c, np.frombuffer(b, np.uint8))
    before = tables(never)
    assert [t[0] for t in before] == [bank.state(c) for c in range(4)]
    assert [t[0][0] == em.ST_LOCKED for t in before] == [True, True, False, False] and all(before[c][1][0] for c in (0, 1))
    assert all(before[c][3] > 0 and before[c][2][4] > 0 for c in (0, 1)), before          # misses and coded blocks counted: their clearing shows
    for c in range(4):          # the emulation goes on from the handle's own tables
        bank.cell[c], bank.link[c], bank.miss[c] = before[c][1], before[c][2], before[c][3]
    assert bank_tables(bank) == before and all(tables(h) == before for h in (plain, heirs, own))
    W, K = R.HANDOVER_DEFAULT_WINDOW, R.HANDOVER_DEFAULT_MAX_SLOTS
    cases = ((plain, [1, 3], lambda h: h.reset_channels([1, 3]), lambda b: (b.reset(1), b.reset(3)), {}),
             (heirs, [2, 3], lambda h: h.handover_channels([2, 3], [0, -1]), lambda b: (b.plant(2, 0, W, K), b.reset(3)), {2: em.PENDING, 3: em.NONE}),
             (own, [0, 2], lambda h: h.resume(137, channels=[0, 2]), lambda b: (b.resume(0, 137, GAP_WINDOW, GAP_MAX_SLOTS), b.resume(2, 137, GAP_WINDOW, GAP_MAX_SLOTS)),
              {0: em.PENDING, 2: em.REFUSED}))
    for h, listed, restart, emulate, status in cases:
        b = copy.deepcopy(bank)
        restart(h)
        emulate(b)
        got, want = tables(h), bank_tables(b)
        for c in range(4):
            assert got[c] == (want[c] if c in listed else before[c]), (listed, c, got[c], want[c], before[c])
        for c in listed:
            assert got[c][2] == [0] * 6 and got[c][3] == 0 and got[c][4][0] == status.get(c, em.NONE), (listed, c, got[c])
    # a donor must be LOCKED: channel 0 of `own` is its own heir now, ASSIST with the status PENDING, and gives nothing
    pending = tables(own)
    own.handover_channels([3], [0])
    b.plant(3, 0, W, K)
    got, want = tables(own), bank_tables(b)
    assert got[3] == want[3] and got[3][4] == (em.REFUSED, 0, 0) and got[3][0] == (em.ST_UNLOCKED, 0, 0, 0) and got[:3] == pending[:3], (got, want)
    assert tables(never) == before
    for h in (plain, heirs, own, never):
        h.close()


@pytest.mark.gpu
def test_gpu_refused_arguments_change_nothing_and_a_handle_without_gaps_is_untouched(pkg, synth):
    """Every refusal of the three entry points: nothing is enqueued, the hand-over status reads NONE (the per-channel fields are not even
    allocated, so the handle still launches the kernels it always did), and every later snapshot -- rows, cell, sync and demodulator state
    -- equals that of a handle that never saw any of the calls.  A wideband handle's chain refuses the chain's entry point."""
    import torch
    R, Wb = pkg.rx_binding, pkg.wbrx_binding
    L = R._lib()
    iq = _three_channels(synth, 0, False)
    X, Z = (pkg.RxChain(3, 16000) for _ in range(2))
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, :6 * TS]))
    arr = lambda v: (C.c_int32 * len(v))(*v)
    ok = R.HandoverParams(8, 72)
    for ch, bits, prm in (([3], 5, ok), ([-1], 5, ok), ([1, 1], 5, ok), ([0, 1, 2, 0], 5, ok), ([1], -1, ok), ([1], 2 ** 31, ok), ([1], 2 ** 40, ok),
                          ([1], 5, R.HandoverParams(128, 72)), ([1], 5, R.HandoverParams(-1, 72)), ([1], 5, R.HandoverParams(8, 0)), ([1], 5, R.HandoverParams(8, 256))):
        assert L.tetra_rx_resume_channels_device(X._h, arr(ch), len(ch), bits, C.byref(prm), None) == ERR_ARG, (ch, bits, prm.window, prm.max_slots)
    assert L.tetra_rx_resume_channels_device(X._h, None, 1, 5, None, None) == ERR_ARG
    assert L.tetra_rx_resume_channels_device(X._h, arr([1]), -1, 5, None, None) == ERR_ARG
    X.resume(5, channels=[])
    assert X.handover_status() == [(0, 0, 0)] * 3
    for h in (X, Z):
        h.process(np.ascontiguousarray(iq[:, 6 * TS:20 * TS]))
    assert _chain_snap(pkg, X, 3) == _chain_snap(pkg, Z, 3)
    X.close(), Z.close()
    xs = torch.zeros((4000, 2), dtype=torch.int16, device="cuda")
    xs[:, 0] = (torch.arange(4000, device="cuda") % 200 - 100).to(torch.int16)
    wb, wz = (pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=2000) for _ in range(2))
    W = Wb._lib()
    g = C.c_int64(-7)
    wb.process_device_at(xs[:1000], 5000)
    wz.process_device(xs[:1000], 1000)
    for n_lost, prm in ((-1, ok), (5, R.HandoverParams(128, 72)), (5, R.HandoverParams(8, 0)), (2 ** 31 * 23, ok), (2 ** 62, ok)):
        assert W.tetra_wbrx_gap(wb._h, n_lost, C.byref(prm), C.byref(g), None) == ERR_ARG and g.value == -7, n_lost
    for x, fmt, n, at, prm, want in ((xs[1000:], 1, 1000, 5999, ok, ERR_ARG), (xs[1000:], 1, 1000, 0, ok, ERR_ARG), (xs[1000:], 3, 1000, 6000, ok, ERR_ARG),
                                     (xs[1000:], -1, 1000, 6000, ok, ERR_ARG), (None, 1, 1000, 6000, ok, ERR_ARG), (xs[1000:], 1, 2001, 6000, ok, ERR_SIZE),
                                     (xs[1000:], 1, -1, 6000, ok, ERR_SIZE), (xs[1000:], 1, 1000, 6100, R.HandoverParams(8, 300), ERR_ARG)):
        rc = W.tetra_wbrx_process_device_at(wb._h, None if x is None else x.data_ptr(), fmt, n, at, C.byref(prm), None)
        assert rc == want, (fmt, n, at, rc)
    assert W.tetra_wbrx_process_device_at(wb._h, xs.data_ptr() + 2, 1, 10, 6000, None, None) == ERR_ALIGN
    assert wb.handover_status() == [(0, 0, 0)] * 3
    wb.process_device_at(xs[1000:2000], 6000)
    wz.process_device(xs[1000:2000], 1000)
    assert _snap(pkg, torch, wb) == _snap(pkg, torch, wz) and wb.handover_status() == [(0, 0, 0)] * 3
    assert L.tetra_rx_resume_channels_device(wb.rx._h, arr([1]), 1, 5, None, None) == ERR_UNSUPPORTED
    with pytest.raises(TypeError):
        wb.rx.resume(5)
    wb.reset()                                         # forgets the origin: any index starts a stream
    wb.process_device_at(xs[:1000], 17)
    assert wb.handover_status() == [(0, 0, 0)] * 3
    wb.close(), wz.close()


# ---------------------------------------------------------------------------------------------------------------------- GPU: wideband

BINS = [BIN_A, BIN_B, BIN_C, BIN_EMPTY]
# 38544 samples at 800 kHz are 1734.48 bits, 3.4 slots: G = 1734, and the exact value falls between two bits
N_LOST = 38544
INDEX_0 = 123456789012                             # a driver's sample index of the capture's first sample


@pytest.fixture(scope="module")
def band(pkg, synth):
    import torch
    return band_capture(torch, synth)


def _gap_run(pkg, torch, xs, mode, stream=None, wait=False, flags=0):
    """The capture in 0.25 s calls.  mode "whole": all of it; "gap": N_LOST samples missing behind call 0 and gap() told so; "untold": the
    same stream, nobody told; "at": the same through process_device_at with the driver's indices, and an overlapping call refused on
    the way; "fresh": the two calls behind the gap, on a new handle.
    -> (per call the per-slot snapshots with the call's demodulated bits, per call the hand-over status, the handle, gap()'s value)"""
    wb = pkg.WidebandRx(BINS, n_channels=M_BAND, decimation=D_BAND, max_in=CALL, flags=flags)
    first = [] if mode == "fresh" else [(0, CALL)]
    calls = first + band_calls(xs.shape[0], CALL if mode == "whole" else CALL + N_LOST)[:2 if mode == "fresh" else None]
    elapsed = []
    before = {1: lambda w: elapsed.append(w.gap(N_LOST, stream=stream))} if mode == "gap" else None

    def at(w, i, a, b):
        if i == 3:
            with pytest.raises(pkg.binding.TetraDemodError) as err:
                w.process_device_at(xs[a - 1:b - 1], INDEX_0 + a - 1, stream=stream)
            assert err.value.status == ERR_ARG
        w.process_device_at(xs[a:b], INDEX_0 + a, stream=stream)

    snaps, status = drive(pkg, torch, wb, xs, calls, before, stream, wait, feed=at if mode == "at" else None, bits=True)
    return snaps, status, wb, elapsed[0] if elapsed else None


@pytest.mark.gpu
def test_gpu_wideband_gap_keeps_code_and_clock(pkg, synth, band):
    """tests/restart_gpu.py's band (A control, B traffic with SYNC bursts in slots 8, 16 and 88, C another cell, one empty bin), N_LOST
    samples dropped at the first call boundary, just behind B's SYNC burst.
      (a) the resampled IQ and the demodulated bits of every slot behind gap() equal a fresh handle's fed the capture behind the gap;
      (b) every row of A, B and C behind the gap equals the uninterrupted run's row of the same kind and TDMA time;
      (c) B's first CRC-good traffic block behind the gap comes before slot 88;
      (d) in the run without gap(), B's CRC-good blocks before slot 88 carry times the uninterrupted run does not have for them (under
          the reference's rule B stays LOCKED and misaligned on normal bursts until a SYNC burst unlocks it, so there are none on this
          band, which (c) is held against; the chain test has such blocks and their times);
      (e) the empty slot reads REFUSED.
    process_device_at with the driver's indices gives the gap() run byte for byte, an overlapping index on the way being refused."""
    import torch
    R = pkg.rx_binding
    xs = band
    whole, _, h0, _ = _gap_run(pkg, torch, xs, "whole")
    told, status, h1, elapsed = _gap_run(pkg, torch, xs, "gap")
    untold, _, h2, _ = _gap_run(pkg, torch, xs, "untold")
    fresh, _, h3, _ = _gap_run(pkg, torch, xs, "fresh")
    at, at_status, h4, _ = _gap_run(pkg, torch, xs, "at")
    assert elapsed == 1734 and abs(N_LOST * 0.045 - 1734.5) < 0.05
    print("hand-over status per call:", status)
    for i, f in enumerate(fresh):                                                          # (a)
        for c in range(4):
            assert told[1 + i][c]["frames"] == f[c]["frames"] and told[1 + i][c]["bits"] == f[c]["bits"], (i, c)
    assert len(fresh) == 2
    assert status[0] == [(0, 0, 0)] * 4                                                    # (e), and the carriers' lock
    for c in range(3):
        assert status[-1][c][0] == 2 and abs(status[-1][c][2]) <= GAP_WINDOW, status[-1]
    assert all(s[3] == (4, 0, 0) for s in status[1:])
    next_sync = B_SYNC_SLOTS[2]
    for slot in range(3):                                                                  # (b)
        want, _ = _blocks_by_time(whole, slot)
        got, order = _blocks_by_time(told, slot, first_call=1)
        assert len(got) == len(order) >= 150, (slot, len(got), len(order))
        for key, val in got.items():
            assert want.get(key) == val, (slot, key, val[:2], want.get(key, (None, None))[:2])
        assert told[-1][slot]["cell"] == whole[-1][slot]["cell"]
    _, order_b = _blocks_by_time(told, 1, first_call=1)
    first_good = min(_slot_index(t) for k, t, ok, ta, bits in order_b if k in TRAFFIC and ok)
    whole_b = {(k, r[5]): r[3] for s in whole for k in TRAFFIC for r in s[1]["rows"][k] if r[2]}
    stale = [(k, r[3], whole_b[(k, r[5])]) for s in untold[1:] for k in TRAFFIC for r in s[1]["rows"][k] if r[2] and (k, r[5]) in whole_b]
    early = [(k, t, tw) for k, t, tw in stale if _slot_index(tw) < next_sync]
    print("B behind the gap: first CRC-good traffic block in TDMA slot %d with gap(); without it %d CRC-good blocks before slot %d, %d of them with the "
          "uninterrupted run's time" % (first_good, len(early), next_sync, sum(t == tw for k, t, tw in early)))
    assert first_good < next_sync                                                          # (c)
    assert all(t != tw for k, t, tw in early)                                              # (d)
    assert at == told and at_status == status                                              # the driver's indices
    for h in (h0, h1, h2, h3, h4):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("one_stream", [False, True])
def test_gpu_gap_with_calls_in_flight(pkg, synth, band, one_stream):
    """process, gap, process ... on a side stream with no wait anywhere (two calls in flight; the two-stream chain and
    TETRA_RX_FLAG_ONE_STREAM) leaves the latest and the previous call's results, frames, all state and the hand-over status equal to the
    same sequence with tetra_rx_wait before and after the gap."""
    import torch
    fl = pkg.rx_binding.FLAG_ONE_STREAM if one_stream else 0
    (_, _, fast, e1), (_, slow_status, slow, e2) = in_flight_and_waited(pkg, torch, lambda stream, wait: _gap_run(pkg, torch, band, "gap", stream=stream, wait=wait, flags=fl))
    assert e1 == e2 == 1734 and fast.handover_status() == slow.handover_status() == slow_status[-1] and [s[0] for s in slow_status[-1]] == [2, 2, 2, 4]
    fast.rx.wait()
    fast.close(), slow.close()


@pytest.mark.gpu
def test_gpu_host_banks_resume_per_shard(pkg):
    """TetraRxBank::resume and the TetraRxMultiBank forwarding (host/tetra_rx_bank.h), 2 shards on one GPU: entries go to the shard that
    holds them in its own numbering, what a shard would refuse is TETRA_ERR_ARG with nothing enqueued on any, the status comes back in the
    bank's channel order.  A plain C++ driver (tests/host/test_gap_bank.cpp)."""
    r = build_and_run_bank_driver(pkg, "test_gap_bank", [7, 2])
    assert r.returncode == 0 and "test_gap_bank: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
