"""The SYNC tracker (k_track in csrc/tetra_lmac.hip, behind tetra_lmac_track_sync_device / _track_sync_lists_device / _track_scramb_device
and through them tetra_rx and tetra_wbrx) against the REFERENCE'S OWN tp_sap_udata_ind: oracle/_ref/libtetra_rxchain_ref.so is the
reference's lower_mac/tetra_lower_mac.c behind its tetra_burst_sync_in / tetra_burst_rx_cb, with the test-side recorder
tests/refrec/tmv_sap_recorder.c below it (oracle/build_ref.sh, oracle/ref_binding.ReferenceRxChain).  Every comparison is exact.

What the reference does with the clock (tetra_lower_mac.c): :172 copies t_phy_state.time to tcd->time on entry of EVERY call, :257-266
overwrite tcd->time's tn / fn / mn only when the SYNC PDU's CRC is good, :268 copies tcd->time back for every SB1.  So an SB1 with a
bad CRC leaves the PHY clock where it was on entry; a good one sets it.

tests/golden/sync_track_golden.npz (make_sync_track_golden.py) holds the inputs below and what the reference recorded for them, for
machines without oracle/_ref."""
import os

import numpy as np
import pytest

from tests.test_lmac import LAYOUTS, _rows_on_device, walk_slots

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sync_track_golden.npz")
N_CALLS = 3


@pytest.fixture(scope="module")
def cref(ref):
    if not (ref.lmac_available() and ref.rxchain_available()):
        pytest.skip("oracle/_ref/libtetra_rxchain_ref.so not built and /root/reference not present")
    return ref


def bad_crc_sb1(ref, t5, rng):
    """The 120 type-5 bits of an SB1 block, corrupted until the reference's own decode (oracle/ref_binding.lmac_decode: its primitives in
    tp_sap_udata_ind's order) reports crc_ok == 0."""
    t5 = t5.copy()
    while True:
        t5[rng.choice(120, 12, replace=False)] ^= 1
        if ref.lmac_decode(ref.TPSAP_T_SB1, t5, ref.SCRAMB_INIT)[1] == 0:
            return t5


def make_case(ref, seed, n_ch, F):
    """Inputs of N_CALLS tracker calls of n_ch channels x F frame slots.  Per slot: does the LOCKED receiver deliver a SYNC burst there
    (valid), its SB1 block's type-5 bits (SYNC PDU fields random over the bit fields' full range: TN 0..3, FN 0..31, MN 0..63; about half
    of them corrupted until the reference reports a bad CRC), and which blocks follow: 1 = a BBK (SYNC burst: after the SB1; any other
    slot: a normal burst's first block), 2 = BBK and SB2, 0 = none (a frame whose burst was not handed over).  nfr: consumed frames per
    call and channel, ragged.  Channel 0 sees no SYNC burst at all, channel 1 starts with bad ones, channel 2 has every slot a SYNC
    burst; a few channels start from a PHY time that is not zero (phy0)."""
    rng = np.random.default_rng(seed)
    valid = (rng.random((N_CALLS, n_ch, F)) < 0.3).astype(np.int32)
    valid[:, 0] = 0
    valid[:, 2] = 1
    bad = rng.random((N_CALLS, n_ch, F)) < 0.5
    bad[0, 1, : F // 2] = True
    follow = rng.choice(np.array([1, 1, 1, 2, 0], np.int32), (N_CALLS, n_ch, F))
    follow[valid == 1] = rng.choice(np.array([1, 2], np.int32), int(valid.sum()))
    nfr = rng.integers(0, F + 1, (N_CALLS, n_ch)).astype(np.int32)
    nfr[:, :3] = F
    nfr[0, 3], nfr[1, 3] = 0, F                   # a call that consumes nothing
    if F > 70:
        nfr[0, 4], nfr[1, 4], nfr[2, 4] = 63, 64, 65   # ends at / just behind the 64-slot group boundary
    t5 = np.zeros((N_CALLS, n_ch, F, 120), np.uint8)
    for k, c, f in np.argwhere(valid == 1):
        row = ref.lmac_encode(ref.TPSAP_T_SB1, rng.integers(0, 2, 60).astype(np.uint8), ref.SCRAMB_INIT)
        t5[k, c, f] = bad_crc_sb1(ref, row, rng) if bad[k, c, f] else row
    phy0 = np.zeros((n_ch, 3), np.uint32)
    phy0[5:8] = [(4, 18, 60), (1, 17, 59), (3, 1, 1)]
    other = rng.integers(0, 2, (N_CALLS, n_ch, F, 216), dtype=np.uint8)          # the BBK's 30 / the SB2's 216 type-5 bits
    return dict(valid=valid, t5=t5, follow=follow, nfr=nfr, phy0=phy0, other=other)


def run_reference(ref, case):
    """The case through the reference: per channel a fresh receiver (zeroed tcd, t_phy_state), per consumed frame one
    tetra_tdma_time_add_tn (tetra_burst_sync.c:113) and then the slot's tp_sap_udata_ind calls in tetra_burst_rx_cb's order.  Recorded
    per slot, from the reference's own objects: entry (t_phy_state.time when the callback would be entered), after (the same after the
    slot's calls), for a SYNC slot the SB1 indication's crc_ok / type-1 bits / tup->tdma_time, for a slot with a following block that
    block's tup->scrambling_code and tup->tdma_time.  final [n_ch][10]: tetra_lmac_cell_state_t as the reference ends (the code from one
    more BBK indication, colour code / MCC / MNC from the crypto state tp_sap_udata_ind keeps beside tcd, tcd time = tup->tdma_time of
    the last SB1 with a good CRC, the PHY time)."""
    valid, t5, follow, nfr, other = case["valid"], case["t5"], case["follow"], case["nfr"], case["other"]
    n_calls, n_ch, F = valid.shape
    z = lambda *s: np.zeros((n_calls, n_ch, F) + s, np.uint32)
    out = dict(entry=z(), after=z(), sb1_ok=z().astype(np.int32), sb1_time=z(), sb1_bits=np.zeros((n_calls, n_ch, F, 60), np.uint8),
               blk_scramb=z(), blk_time=z(), final=np.zeros((n_ch, 10), np.uint32))
    for c in range(n_ch):
        rx = ref.ReferenceRxChain()
        rx.set_phy_time(*case["phy0"][c])
        tcd_time, seen_sb1 = (0, 0, 0), False
        for k in range(n_calls):
            for f in range(min(int(nfr[k, c]), F)):
                rx.add_tn(1)
                out["entry"][k, c, f] = ref.tdma_pack(*rx.phy_time())
                if valid[k, c, f]:
                    rx.udata_ind(ref.TPSAP_T_SB1, 1, t5[k, c, f])
                if follow[k, c, f]:
                    rx.udata_ind(ref.TPSAP_T_BBK, 0, other[k, c, f])
                if follow[k, c, f] == 2:
                    rx.udata_ind(ref.TPSAP_T_SB2, 2, other[k, c, f])
                ev = rx.events()
                assert len(ev) == int(valid[k, c, f]) + int(follow[k, c, f])
                if valid[k, c, f]:
                    e = ev.pop(0)
                    assert e["lchan"] == ref.TETRA_LC_BSCH and e["blk_num"] == 1 and e["scramb"] == ref.SCRAMB_INIT and e["bits"].size == 60
                    out["sb1_ok"][k, c, f], out["sb1_time"][k, c, f], out["sb1_bits"][k, c, f] = e["crc_ok"], e["time"], e["bits"]
                    seen_sb1 = True
                    if e["crc_ok"]:
                        tcd_time = (e["time"] & 0xff, (e["time"] >> 8) & 0xff, e["time"] >> 16)
                if ev:
                    assert ev[0]["lchan"] == ref.TETRA_LC_AACH
                    out["blk_scramb"][k, c, f], out["blk_time"][k, c, f] = ev[0]["scramb"], ev[0]["time"]
                    assert all(e["scramb"] == ev[0]["scramb"] and e["time"] == ev[0]["time"] for e in ev)
                out["after"][k, c, f] = ref.tdma_pack(*rx.phy_time())
        rx.udata_ind(ref.TPSAP_T_BBK, 0, other[0, c, 0])
        code = rx.events()[0]["scramb"]
        mcc, mnc, cc, _ = rx.network()
        assert seen_sb1 or (mcc, mnc, cc) == (0, 0, 0)
        out["final"][c] = [code, cc, mcc, mnc, *tcd_time, *rx.phy_time()]
        rx.close()
    return out


def tracker_inputs(case, rec, k):
    """Call k as the tracker takes it, every array from the reference's run: decoded SB1 rows [n_ch * F][80] (the type-1 bits the
    reference handed up; the tracker reads bits 0..55), crc_ok, valid, consumed frames."""
    n_calls, n_ch, F = case["valid"].shape
    t2 = np.zeros((n_ch * F, 80), np.uint8)
    t2[:, :60] = rec["sb1_bits"][k].reshape(n_ch * F, 60)
    return t2, rec["sb1_ok"][k].reshape(-1).astype(np.int32), case["valid"][k].reshape(-1).astype(np.int32), case["nfr"][k].astype(np.int32)


def start_cells(case):
    cell = np.zeros((case["valid"].shape[1], 10), np.uint32)
    cell[:, 7:10] = case["phy0"]
    return cell


def check_against_reference(case, rec, k, scr, t_rx, t_af, label):
    """One call's per-slot tracker outputs == what the reference recorded.  Slots past a channel's consumed frames: times 0.
    t_rx = t_af = None: the codes alone (tetra_lmac_track_scramb_device has no clock)."""
    n_calls, n_ch, F = case["valid"].shape
    scr = np.asarray(scr, np.uint32).reshape(n_ch, F)
    live = np.arange(F)[None, :] < case["nfr"][k][:, None]
    sync = live & (case["valid"][k] == 1)
    blk = live & (case["follow"][k] > 0)

    def same(got, want, where, what):
        bad = np.argwhere((got != want) & where)
        assert bad.size == 0, (f"{label} call {k}: {what} differs first at channel {bad[0][0]} slot {bad[0][1]}: got {int(got[tuple(bad[0])]):#x}, "
                               f"the reference {int(want[tuple(bad[0])]):#x} ({len(bad)} slots in all)")
    same(scr, rec["blk_scramb"][k], blk, "scrambling code")
    if t_rx is None:
        return
    t_rx, t_af = (np.asarray(a, np.uint32).reshape(n_ch, F) for a in (t_rx, t_af))
    same(t_rx, rec["entry"][k], live, "time on entry")
    same(t_af, rec["after"][k], live, "PHY time after the slot")
    same(t_af, rec["sb1_time"][k], sync, "tup->tdma_time of the SB1")
    same(t_af, rec["blk_time"][k], blk, "tup->tdma_time of the block after the SB1")
    same(t_rx, np.zeros_like(t_rx), ~live, "time on entry of an unused slot")
    same(t_af, np.zeros_like(t_af), ~live, "time of an unused slot")


def case_preconditions(case, rec):
    """The case holds what the issue is about: bad-CRC SB1s after good ones whose PDU time is not the clock's, and group boundaries."""
    n_calls, n_ch, F = case["valid"].shape
    n_bad_after_good = 0
    for c in range(n_ch):
        good_time = None
        for k in range(n_calls):
            for f in range(min(int(case["nfr"][k, c]), F)):
                if not case["valid"][k, c, f]:
                    continue
                if rec["sb1_ok"][k, c, f]:
                    good_time = rec["sb1_time"][k, c, f]
                elif good_time is not None and rec["after"][k, c, f] != good_time:
                    n_bad_after_good += 1
    assert n_bad_after_good >= 20
    ok = rec["sb1_ok"][case["valid"] == 1]
    assert 0.25 < ok.mean() < 0.75


# (seed, channels, frame slots per call): three 64-slot groups with a ragged last one; one short of / exactly / one past a group
CASES = ((41, 12, 150), (42, 9, 63), (43, 9, 64), (44, 9, 65))
GOLDEN_CASES = ((51, 9, 70), (52, 8, 29))           # what the committed fixture holds: 9 * 70 * 3 + 8 * 29 * 3 frame slots


def test_walk_slots_equals_the_reference_lower_mac(cref):
    """2(a): tests/test_lmac.walk_slots -- what every tracker test in test_lmac.py compares the kernel with -- against the reference's own
    tp_sap_udata_ind, slot by slot: scrambling code, time on entry, tup->tdma_time of the SB1 and of the block after it, final state."""
    for seed, n_ch, F in CASES:
        case = make_case(cref, seed, n_ch, F)
        rec = run_reference(cref, case)
        case_preconditions(case, rec)
        cell = start_cells(case)
        for k in range(N_CALLS):
            t2, ok, valid, nfr = tracker_inputs(case, rec, k)
            scr, t_rx, t_af = walk_slots(cref, cell, t2, ok, valid, nfr)
            check_against_reference(case, rec, k, scr, t_rx, t_af, f"walk_slots seed {seed}")
        assert np.array_equal(cell, rec["final"]), (seed, np.argwhere(cell != rec["final"])[:4])


def test_rxchain_library_is_self_contained(cref):
    """The first trap of the build: oracle/ref_binding loads tests/refrec/tp_sap_recorder.c RTLD_GLOBAL, and that recorder defines
    tp_sap_udata_ind too.  libtetra_rxchain_ref.so must call its OWN (the reference's) and use its OWN t_phy_state whatever was loaded
    before it, and two receivers must not share tcd or the clock."""
    import ctypes as C
    if not cref.sync_run_available():
        pytest.skip("oracle/_ref recorder library not built")
    old = cref.ReferenceBurstSync()                                       # loads the RTLD_GLOBAL recorder and libtetra_burst_ref.so
    glob_udata = C.cast(cref._rec_lib().tp_sap_udata_ind, C.c_void_p).value
    glob_phy = C.addressof(C.c_char.in_dll(cref.lib(), "t_phy_state"))
    a, b = cref.ReferenceRxChain(), cref.ReferenceRxChain()
    (ua, pa), (ub, pb) = a.own_addresses(), b.own_addresses()
    assert len({ua, ub, glob_udata}) == 3 and len({pa, pb, glob_phy}) == 3
    # a SYNC burst through a's tetra_burst_sync_in: the indications arrive at a's recorder (through the reference's tp_sap_udata_ind: they
    # carry decoded type-1 bits and a CRC verdict), nothing at the global recorder, nothing at b
    rng = np.random.default_rng(3)
    t1 = rng.integers(0, 2, 60).astype(np.uint8)
    burst = cref.build_sync_burst(cref.lmac_encode(cref.TPSAP_T_SB1, t1, cref.SCRAMB_INIT), rng.integers(0, 2, 30), rng.integers(0, 2, 216))
    a.feed(np.concatenate([burst] * 6))
    ev = a.events()
    assert len(ev) >= 6 and ev[0]["lchan"] == cref.TETRA_LC_BSCH and ev[0]["crc_ok"] == 1 and np.array_equal(ev[0]["bits"], t1)
    assert old.feed(np.zeros(0, np.uint8)) == [] and b.events() == []
    assert a.phy_time() != (0, 0, 0) and b.phy_time() == (0, 0, 0)
    # tcd is per copy: b's first non-SB1 block is still descrambled with a zero code
    b.udata_ind(cref.TPSAP_T_BBK, 0, np.zeros(30, np.uint8))
    a.udata_ind(cref.TPSAP_T_BBK, 0, np.zeros(30, np.uint8))
    val = lambda lo, n: int("".join(str(int(x)) for x in t1[lo:lo + n]), 2)
    assert b.events()[0]["scramb"] == 0 and a.events()[0]["scramb"] == cref.scramb_get_init(val(31, 10), val(41, 14), val(4, 6))
    for x in (a, b, old):
        x.close()


# ---------------------------------------------------------------------------------------------------------------------
# The committed fixture: the same inputs and what the reference recorded for them, for machines without oracle/_ref
# ---------------------------------------------------------------------------------------------------------------------
GOLDEN_REC_KEYS = ("entry", "after", "sb1_ok", "sb1_time", "sb1_bits", "blk_scramb", "blk_time", "final")


def load_golden():
    """-> [(case, rec)] as make_case / run_reference return them (t5 only; the following blocks' own bits are not stored)."""
    g = np.load(GOLDEN)
    out = []
    for i in range(int(g["n_cases"])):
        valid = g[f"valid_{i}"]
        t5 = np.unpackbits(g[f"t5_packed_{i}"], axis=-1)[..., :120]
        case = dict(valid=valid, follow=g[f"follow_{i}"], nfr=g[f"nfr_{i}"], phy0=g[f"phy0_{i}"], t5=t5)
        rec = {k: g[f"{k}_{i}"] for k in GOLDEN_REC_KEYS}
        rec["sb1_bits"] = np.unpackbits(rec["sb1_bits"], axis=-1)[..., :60]
        out.append((case, rec))
    return out


def test_golden_is_what_the_reference_gives_now(cref):
    """The fixture is current: the reference, built here, records the same events for the fixture's inputs."""
    gold = load_golden()
    assert len(gold) == len(GOLDEN_CASES)
    for (seed, n_ch, F), (gcase, grec) in zip(GOLDEN_CASES, gold):
        case = make_case(cref, seed, n_ch, F)
        for k in ("valid", "follow", "nfr", "phy0", "t5"):
            assert np.array_equal(case[k], gcase[k]), (seed, k)
        rec = run_reference(cref, case)
        for k in GOLDEN_REC_KEYS:
            assert np.array_equal(rec[k], grec[k]), (seed, k)


def live_and_golden(ref_or_none):
    cases = list(load_golden())
    if ref_or_none is not None:
        for seed, n_ch, F in CASES:
            case = make_case(ref_or_none, seed, n_ch, F)
            cases.append((case, run_reference(ref_or_none, case)))
    return cases


def run_host_rule(case, rec, stale=False):
    """2(c): the kernel's own rule (lmac_core.hpp track_slot / track_carry, the functions k_track calls, built for the host by
    tests/emul/lmac_emul.cpp) over 64-slot groups, three calls with carried state, checked against the reference's record."""
    from tests.emul import lmac_emul_bind
    cell = start_cells(case)
    for k in range(N_CALLS):
        t2, ok, valid, nfr = tracker_inputs(case, rec, k)
        scr, t_rx, t_af = lmac_emul_bind.track(t2, ok, valid, nfr, cell, stale_tcd_on_bad_crc=stale)
        check_against_reference(case, rec, k, scr, t_rx, t_af, "host rule" + (" (planted fault)" if stale else ""))
    assert np.array_equal(cell, rec["final"]), np.argwhere(cell != rec["final"])[:4]


def test_host_rule_equals_golden():
    """The kernel's rule on the host == the reference's record in the committed fixture (70 slots: a group boundary with consumed
    frames ending inside the second group; a channel without any SYNC burst)."""
    gold = load_golden()
    for case, rec in gold:
        case_preconditions(case, rec)
        run_host_rule(case, rec)
    assert gold[0][0]["valid"].shape[2] > 64 and not gold[0][0]["valid"][:, 0].any()


def test_host_rule_equals_the_reference_lower_mac(cref):
    """... and the live reference: 150 slots per call (three groups, a ragged last one), 63 / 64 / 65 slots (the group boundary at slots 63
    and 64), consumed frames ending inside a group (63, 64, 65 of 150; random counts), a channel with no SYNC burst at all."""
    for case, rec in live_and_golden(cref)[len(GOLDEN_CASES):]:
        run_host_rule(case, rec)


def test_planted_fault_stale_tcd_time_is_caught():
    """2(d): the host rule with the earlier behaviour switched back on -- an SB1 with a bad CRC sets the clock to the time of the last
    good SYNC PDU -- fails the very check of 2(c), on the fixture alone."""
    for case, rec in load_golden():
        with pytest.raises(AssertionError, match="planted fault"):
            run_host_rule(case, rec, stale=True)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the three tracker entry points on the same inputs
# ---------------------------------------------------------------------------------------------------------------------
def run_gpu_trackers(pkg, case, rec, label):
    import torch
    lb, bb = pkg.lmac_binding, pkg.bsync_binding
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    n_calls, n_ch, F = case["valid"].shape
    n = n_ch * F
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cell0 = start_cells(case)
    cell_slot, cell_list = d(cell0.view(np.int32)), d(cell0.view(np.int32).copy())
    d_code = torch.zeros(n_ch, dtype=torch.int32, device=dev)
    for k, (stride, offset) in zip(range(n_calls), LAYOUTS):
        t2, ok, valid, nfr = tracker_inputs(case, rec, k)
        live = (np.arange(F)[None, :] < nfr[:, None]).reshape(-1)
        # slot layout: a row per frame slot, this call's row stride and alignment
        outs = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)]
        lb.track_sync_device(_rows_on_device(t2, stride, offset, rng), stride, d(ok), d(valid), d(nfr), n_ch, F, cell_slot, *outs)
        # compact rows: one per SYNC-typed slot (also those past the consumed frames: typed, but not frames), 4-byte aligned
        types = np.where(valid == 1, 3, rng.choice(np.array([0, 1, -1], np.int32), n)).astype(np.int32)
        sync = np.flatnonzero(types == 3)
        d_ft = d(types)
        lists = torch.zeros((4, n), dtype=torch.int32, device=dev)
        counts = torch.zeros(4, dtype=torch.int32, device=dev)
        chan_first = torch.zeros((4, n_ch), dtype=torch.int32, device=dev)
        bb.index_device(d_ft, F, lists, counts, chan_first)
        outs_l = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)]
        bitnum = torch.arange(n, dtype=torch.int32, device=dev) * 5
        labels = torch.full((n, 6), -1, dtype=torch.int32, device=dev)
        lb.track_sync_lists_device(d(np.concatenate([t2[sync], np.zeros((1, 80), np.uint8)])), 80, d(np.concatenate([ok[sync], [0]]).astype(np.int32)), d_ft,
                                   d(nfr), chan_first[0], n_ch, F, cell_list, *outs_l, d_frame_bitnum=bitnum, d_sb1_labels=labels)
        # the code alone: every slot counts there, so the slots past the consumed frames are handed over as holding no SB1
        d_rows = torch.zeros(n, dtype=torch.int32, device=dev)
        lb.track_scramb_device(_rows_on_device(t2, stride, offset, rng), stride, d(ok), d((valid * live).astype(np.int32)), n_ch, F, d_code, d_rows)
        torch.cuda.synchronize()
        for name, o in (("track_sync_device", outs), ("track_sync_lists_device", outs_l)):
            check_against_reference(case, rec, k, *(x.cpu().numpy().view(np.uint32) for x in o), f"{label} {name}")
        check_against_reference(case, rec, k, d_rows.cpu().numpy().view(np.uint32), None, None, f"{label} track_scramb_device")
        lab = labels.cpu().numpy()
        for j, r in enumerate(sync):
            c, f = divmod(int(r), F)
            if f < nfr[c]:
                assert list(lab[j].view(np.uint32)) == [c, f, 5 * r, rec["entry"][k, c, f], rec["sb1_time"][k, c, f], rec["sb1_ok"][k, c, f]], (label, k, c, f)
            else:
                assert (lab[j] == -1).all()
        assert (lab[sync.size:] == -1).all()
    for name, cell in (("track_sync_device", cell_slot), ("track_sync_lists_device", cell_list)):
        got = cell.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, rec["final"]), (label, name, np.argwhere(got != rec["final"])[:4])
    assert np.array_equal(d_code.cpu().numpy().view(np.uint32), rec["final"][:, 0]), label


@pytest.mark.gpu
def test_gpu_trackers_equal_golden(pkg):
    """4(a) on the committed fixture: tetra_lmac_track_sync_device, _track_sync_lists_device and _track_scramb_device -- three calls with
    carried state, ragged frame counts, the row layouts of LAYOUTS -- give the reference's recorded codes, times, labels and cell state."""
    for i, (case, rec) in enumerate(load_golden()):
        run_gpu_trackers(pkg, case, rec, f"golden {i}")


@pytest.mark.gpu
def test_gpu_trackers_equal_the_reference_lower_mac(pkg, cref):
    """4(a) against the reference run of the inputs of 2(a)."""
    for (seed, _, _), (case, rec) in zip(CASES, live_and_golden(cref)[len(GOLDEN_CASES):]):
        run_gpu_trackers(pkg, case, rec, f"seed {seed}")


# ---------------------------------------------------------------------------------------------------------------------
# The whole chain against the reference's whole chain, on a stream with failures in it
# ---------------------------------------------------------------------------------------------------------------------
FAIL_SLOTS = 140
FAIL_BAD_SB1 = (36, 40, 60, 64, 100, 104, 124)     # SYNC bursts whose SB1 fails its CRC; 40 / 64 / 104: the last good SYNC PDU is 8 frames back
FAIL_GARBAGE = (78, 79, 80, 81)                    # consecutive bursts replaced by random bits: the receiver unlocks and locks again
FAIL_CELLS = ((262, 1, 5), (901, 16383, 63), (1, 2, 0))
SB_BLK1_OFFSET = 94                                # tetra_burst.c:33


def failure_stream(ref, synth, c):
    """Channel c's transmit bits: synth.gen_downlink, altered deterministically -- see FAIL_BAD_SB1 / FAIL_GARBAGE; the training
    sequences of the bad-SB1 bursts stay intact."""
    rng = np.random.default_rng(900 + c)
    bits = synth.gen_downlink(FAIL_SLOTS, 7000 + c, cell=FAIL_CELLS[c])[0].reshape(FAIL_SLOTS, 510).copy()
    for s in FAIL_BAD_SB1:
        assert s % 4 == 0
        bits[s, SB_BLK1_OFFSET:SB_BLK1_OFFSET + 120] = bad_crc_sb1(ref, bits[s, SB_BLK1_OFFSET:SB_BLK1_OFFSET + 120], rng)
    for s in FAIL_GARBAGE:
        bits[s] = rng.integers(0, 2, 510)
    return bits.reshape(-1)


KIND_OF_BURST = {("sync", 0): 0, ("sync", 1): 1, ("sync", 2): 2, ("norm2", 0): 1, ("norm2", 1): 3, ("norm2", 2): 4, ("norm1", 0): 1, ("norm1", 1): 5}


def reference_rows(ref, bits):
    """`bits` through the reference's whole chain, a bit per tetra_burst_sync_in call (what the product's synchroniser reproduces) ->
    (rows, facts).  rows: per handed-over block (kind as pkg.rx_binding numbers them, bitnum, crc_ok, time on entry, tup->tdma_time, type-1
    bits), in the reference's order.  The time on entry of tetra_burst_rx_cb is the PHY time before the frame plus one
    tetra_tdma_time_add_tn (the reference's own), cross-checked against curr_frame / curr_multiframe, which tetra_burst.c:349-350 store on
    entry.  facts: per SB1 (bitnum, crc_ok, tup time, PHY time after, PHY time on entry) and the receiver's state after every frame."""
    from tests.chain_host import TdmaTime as _TdmaTime, ref_add_tn as _ref_add_tn
    import ctypes as C
    add_tn = _ref_add_tn(ref)
    rx = ref.ReferenceRxChain()
    rows, sb1, states = [], [], []
    for before, state_after, ev in rx.feed_bitwise(bits):
        states.append(state_after)
        if not ev:
            continue
        t = _TdmaTime(tn=before[0], fn=before[1], mn=before[2])
        add_tn(C.byref(t), 1)
        entry = ref.tdma_pack(t.tn, t.fn, t.mn)
        assert all(e["curr_frame"] == t.fn and e["curr_multiframe"] == t.mn and e["bitnum"] == ev[0]["bitnum"] for e in ev)
        if ev[0]["lchan"] == ref.TETRA_LC_BSCH:
            burst = "sync"
            assert [(e["bits"].size, e["blk_num"]) for e in ev] == [(60, 1), (14, 0), (124, 2)]
            sb1.append((ev[0]["bitnum"], ev[0]["crc_ok"], ev[0]["time"], ev[0]["phy"], entry))
        elif len(ev) == 3:
            burst = "norm2"
            assert [(e["bits"].size, e["blk_num"]) for e in ev] == [(14, 0), (124, 1), (124, 2)]
        else:
            burst = "norm1"
            assert [(e["bits"].size, e["blk_num"]) for e in ev] == [(14, 0), (268, 0)]
        for i, e in enumerate(ev):
            rows.append((KIND_OF_BURST[(burst, i)], e["bitnum"], e["crc_ok"], entry, e["time"], e["scramb"], e["bits"].tobytes()))
    rx.close()
    return rows, dict(sb1=sb1, states=states)


def failure_preconditions(ref, rows, facts):
    """The reference run holds the cases the test is for (so that it cannot pass emptily): >= 3 SB1 with a bad CRC while LOCKED whose last
    good SYNC PDU is >= 8 frames back, the PHY time after each differing from that PDU's time; an UNLOCKED -> LOCKED transition after the
    first lock; >= 200 blocks to compare."""
    stale, last_good = 0, None
    for bitnum, ok, tup_time, phy_after, entry in facts["sb1"]:
        if ok:
            last_good = (bitnum, tup_time)
        elif last_good is not None and bitnum - last_good[0] >= 8 * 510:
            assert phy_after != last_good[1] and phy_after == entry
            stale += 1
    assert stale >= 3, stale
    st = [s for s in facts["states"]]
    first_lock = st.index(ref.RX_S_LOCKED)
    relock = [i for i in range(first_lock + 1, len(st)) if st[i] == ref.RX_S_LOCKED and st[i - 1] != ref.RX_S_LOCKED
              and ref.RX_S_UNLOCKED in st[first_lock:i]]
    assert relock, "no UNLOCKED -> LOCKED transition after the first lock"
    assert len(rows) >= 200, len(rows)


def test_failure_stream_holds_its_cases_on_the_transmit_bits(cref, synth):
    """Before any GPU is used: the altered transmit bits themselves, through the reference's chain, hold the bad-CRC SB1s while LOCKED
    and the loss of lock that 4(b) is about."""
    for c in range(len(FAIL_CELLS)):
        rows, facts = reference_rows(cref, failure_stream(cref, synth, c))
        failure_preconditions(cref, rows, facts)
        bad = [s for s in facts["sb1"] if not s[1]]
        assert len(bad) >= len(FAIL_BAD_SB1) - 1


@pytest.mark.gpu
def test_gpu_rx_chain_equals_the_reference_chain_on_a_stream_with_failures(pkg, cref, synth):
    """4(b): per channel a coded downlink at the usual 25 dB with SYNC bursts whose SB1 fails its CRC and a stretch of lost bursts,
    through pkg.RxChain in ragged calls.  The demodulated bits the chain itself produced go to the reference's whole chain
    (tetra_burst_sync_in -> tetra_burst_rx_cb -> tp_sap_udata_ind); every row the handle returns equals the matching reference
    indication -- kind, bit number, crc_ok, type-1 bits, tdma_time (tup->tdma_time), tdma_time_rx (the PHY time on entry of
    tetra_burst_rx_cb) -- and there is a row for every indication.  Both sides consume identical bits: nothing is excluded."""
    import torch
    from tests.chain_gpu import bit_rows as _bit_rows
    R = pkg.rx_binding
    Cn = len(FAIL_CELLS)
    N = FAIL_SLOTS * 510 - 100
    tx = [failure_stream(cref, synth, c) for c in range(Cn)]
    for c in range(Cn):                                     # on the CPU first
        failure_preconditions(cref, *reference_rows(cref, tx[c]))
    iq = np.stack([synth.gen_channel(N, 7100 + c, bits=tx[c])[0] for c in range(Cn)])
    cuts = [0, 9000, 9001, 20000, 20180, 33000, 47111, 60000, N]
    rx = pkg.RxChain(Cn, 16000)
    got = [[] for _ in range(Cn)]
    demod = [b"" for _ in range(Cn)]
    for a, b in zip(cuts, cuts[1:]):
        rx.process(np.ascontiguousarray(iq[:, a:b]))
        rx.wait()
        for k in range(R.N_KINDS):
            blocks, t1 = rx.fetch(k)
            for j, blk in enumerate(blocks):
                got[int(blk["channel"])].append((int(blk["bitnum"]), k, int(blk["crc_ok"]), int(blk["tdma_time_rx"]), int(blk["tdma_time"]), t1[j].tobytes()))
        for c, row in enumerate(_bit_rows(torch, rx, Cn)):
            demod[c] += row
    cells = rx.cells()
    rx.close()
    for c in range(Cn):
        bits = np.frombuffer(demod[c], np.uint8)
        assert bits.size > N - 600
        rows, facts = reference_rows(cref, bits)
        failure_preconditions(cref, rows, facts)
        want = sorted((bitnum, kind, ok, entry, time, t1) for kind, bitnum, ok, entry, time, scramb, t1 in rows)
        have = sorted(got[c])
        assert len(have) == len(want), (c, len(have), len(want))
        for h, w in zip(have, want):
            assert h[:5] == w[:5] and h[5][:len(w[5])] == w[5], (c, "bitnum %d kind %d" % h[:2], [hex(x) for x in h[2:5]], [hex(x) for x in w[2:5]])
        # the code in force at the end is the one the reference used last, and the clock is the reference's
        assert cells[c].scramb_init == [r[5] for r in rows if r[0] != R.KIND_SB1][-1]
    # 4(c), the same stream through WidebandRx, is left out: test_wbrx.py's small_capture builds its carriers' bits itself and takes none
    # from the caller.
