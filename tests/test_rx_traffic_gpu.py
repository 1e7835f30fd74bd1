"""The traffic routing of the receive chain (include/ext/tetra_traffic.h) on the GPU, against tests/traffic_definition.py: the walk of
tests/chain_host.py over the oracle's frames under the reference's decoder, clock and codes, the rule restated from the reference's
lines, and the reference's own functions chained on the routed frames.  Every comparison is exact.

The stream: 4 channels x 40 slots from slot 60 on (frames 16, 17, 18, 1 .. 7), 20 400 samples, in tests/chain_gpu.ragged_cuts pieces
(9000, 180, 1, 0, 4000, ...: the longest piece sets the handle's max_samples) with the results fetched one call late."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import chain_gpu as G
from tests import soft_pipeline as SP
from tests import tch_definition as td
from tests import traffic_definition as T

pytestmark = pytest.mark.gpu
ARG, UNSUPPORTED, SIZE = -1, -2, -6
CUTS = G.ragged_cuts(T.SAMPLES)
MAX_SAMPLES = max(b - a for a, b in zip(CUTS, CUTS[1:]))
_cache = {}


def _need_ref(ref):
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not available")


def _mixed(synth, oracle):
    """the mixed table's stream, made once: (cells, tx, iq, the oracle's bits and soft values)"""
    if "mixed" not in _cache:
        cells, tx, iq = T.downlink(synth, T.MIXED)
        iq.flags.writeable = False
        _cache["mixed"] = (cells, tx, iq, SP.oracle_streams(oracle, iq))
    return _cache["mixed"]


def _want_mixed(ref, oracle, synth, flags):
    key = ("want", flags & (T.SOFT | T.BITERR | T.AACH_RM3014 | T.AACH_SOFT))
    if key not in _cache:
        _, _, iq, streams = _mixed(synth, oracle)
        _cache[key] = T.stream_rows(ref, oracle, iq, T.MIXED, key[1], streams)
    return _cache[key]


def _traffic_rows(rx, R, which, biterr):
    """{kind: [(channel, bitnum, crc_ok, time on entry, time, type-2 bytes, count word or None)]}, and the rows dropped per kind"""
    out, dropped = {}, {}
    for k in T.TCH_KINDS:
        got = rx.fetch_traffic(k, which, biterr=biterr and k in td.CODED)
        blocks, t2, dropped[k] = got[:3]
        words = got[3] if len(got) > 3 else [None] * len(blocks)
        out[k] = [r + (None if w is None else int(w),) for r, w in zip(G.rows(blocks, t2), words)]
    return out, dropped


def _run(pkg, iq, table, flags=0, cuts=CUTS, max_samples=MAX_SAMPLES, max_rows=None, enable=True, change=None):
    """The stream through one handle in overlapping calls, results fetched one call late -> (traffic rows per call [{kind: rows}], rows
    dropped per call, the six kinds' rows per call, cells, links or None).  table: table_of's form, set before the first call;
    change = (k, table): set behind call k's enqueue, with call k still in flight."""
    import torch
    R = pkg.rx_binding
    dev = torch.device("cuda", 0)
    d_iq = torch.from_numpy(np.array(iq)).to(dev)
    rx = pkg.RxChain(iq.shape[0], max_samples, flags=flags)
    biterr = bool(flags & R.FLAG_BITERR)
    try:
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        if enable:
            rx.enable_traffic(max_rows)
            rx.set_traffic(T.table_arg(table), stream=s)
        calls, drops, six = [], [], []

        def take(which):
            rows, dropped = _traffic_rows(rx, R, which, biterr) if enable else ({}, {})
            calls.append(rows), drops.append(dropped), six.append(G.collect(rx, R, which))
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            G.enqueue(torch, rx, d_iq, a, b, s)
            if change and change[0] == i:
                rx.set_traffic(T.table_arg(change[1]), stream=s)
            if i >= 1:
                take(1)
        take(0)
        rx.wait()
        cells = [bytes(c) for c in rx.cells()]
        links = rx.links() if biterr else None
    finally:
        rx.close()
    return calls, drops, six, cells, links


def _flat(calls):
    return {k: [r for c in calls for r in c[k]] for k in T.TCH_KINDS}


def _by_channel(rows):
    """rows of all calls in the definition's order: channel-major, frames in order"""
    return {k: sorted(v, key=lambda r: (r[0], r[1])) for k, v in rows.items()}


def test_gpu_traffic_mixed_table_on_one_stream_and_on_two(pkg, synth, oracle, ref):
    """A table that mixes all three kinds, off timeslots and gated and ungated entries across the channels, at the synth's default
    level: rows, labels and counts are the definition's bit for bit, with the tail on a stream of its own and on the caller's; within a
    call a kind's rows are in (channel, frame) order; nothing is dropped; every payload is the one that was sent."""
    _need_ref(ref)
    R = pkg.rx_binding
    cells, tx, iq, _ = _mixed(synth, oracle)
    want = _want_mixed(ref, oracle, synth, 0)
    assert {k: len(v) for k, v in want.items()} == {8: 14, 9: 14, 10: 15}
    for flags in (0, R.FLAG_ONE_STREAM):
        calls, drops, six, _, _ = _run(pkg, iq, T.MIXED, flags)
        assert len(calls) == len(CUTS) - 1
        for c in calls:
            for k, rows in c.items():
                assert [(r[0], r[1]) for r in rows] == sorted((r[0], r[1]) for r in rows), (flags, k)
        assert all(d == {8: 0, 9: 0, 10: 0} for d in drops)
        got = _by_channel(_flat(calls))
        for k in T.TCH_KINDS:
            assert got[k] == want[k], (flags, k, len(got[k]), len(want[k]))
        T.assert_payloads(got, tx)
        # the routed slot's SCH/F row is still delivered (CRC-bad: it is no SCH/F block)
        schf = {(r[0], r[1]): r[2] for c in six for r in c[R.KIND_SCH_F]}
        assert all((r[0], r[1]) in schf for k in got for r in got[k]) and sum(schf[(r[0], r[1])] for k in got for r in got[k]) == 0


def _gate_stream(synth):
    """c0: the transmitter names marker 9, the receiver waits for 10.  c1: header 0 with the right field 1.  c2: the right PDU with four
    planted bit errors, which the RM(30,14) decoder gives up on.  c3: an open gate (marker 63 sent and expected)."""
    cw = T.codewords()
    bits = lambda word: np.array([(int(word) >> (29 - i)) & 1 for i in range(30)], np.uint8)
    hdr0 = np.tile(bits(cw[0 << 12 | 33 << 6]), (T.SLOTS, 1))
    broken = bits(cw[1 << 12 | 20 << 6])
    broken[[3, 11, 17, 29]] ^= 1
    aach = [None, hdr0, np.tile(broken, (T.SLOTS, 1)), None]
    sent = T.table_of(4, {(0, 4): (9, 9), (1, 2): (10, 0), (2, 2): (9, 0), (2, 4): (8, 0), (3, 2): (10, 63)})
    gated = T.table_of(4, {(0, 4): (9, 10), (1, 2): (10, 33), (2, 2): (9, 20), (2, 4): (8, 20), (3, 2): (10, 63)})
    open_ = T.table_of(4, {(0, 4): (9, 0), (1, 2): (10, 0), (2, 2): (9, 0), (2, 4): (8, 0), (3, 2): (10, 0)})
    return T.downlink(synth, sent, aach=aach), gated, open_


def test_gpu_traffic_usage_gate(pkg, synth, oracle, ref):
    """Under TETRA_RX_FLAG_AACH_RM3014: a wrong marker, header 0 with the right field 1 and a BBK row made undecodable (4 planted errors)
    each route nothing, while the ungated twin of each entry routes the slot; an entry whose marker is the one sent routes either way.
    Both runs are the definition's rows."""
    _need_ref(ref)
    R = pkg.rx_binding
    (cells, tx, iq), gated, open_ = _gate_stream(synth)
    streams = SP.oracle_streams(oracle, iq)
    got = {}
    for name, table in (("gated", gated), ("open", open_)):
        calls, drops, six, _, _ = _run(pkg, iq, table, R.FLAG_AACH_RM3014)
        got[name] = _by_channel(_flat(calls))
        want = T.stream_rows(ref, oracle, iq, table, T.AACH_RM3014, streams)
        assert got[name] == want, name
        if name == "gated":      # the undecodable rows are there, with the decoder's verdict
            bbk = [r for c in six for r in c[R.KIND_BBK] if r[0] == 2]
            assert sum(1 for r in bbk if r[2] == 0) > 20
    per = lambda rows, c: sum(1 for k in rows for r in rows[k] if r[0] == c)
    assert [per(got["gated"], c) for c in range(4)] == [0, 0, 0, per(got["open"], 3)]
    assert all(per(got["open"], c) >= 4 for c in range(4)), [per(got["open"], c) for c in range(4)]
    T.assert_payloads(got["open"], tx)


def test_gpu_traffic_exclusions(pkg, synth, oracle, ref):
    """No row for: the frame-18 slots of a traffic timeslot; a NORM_2 burst planted in a traffic timeslot (a stolen slot: its NDB 1 / 2
    rows are there as ever, with good CRCs and the planted bits); the slots of a channel whose first SB1 is corrupted, so that frames
    exist before any SYNC PDU with a good CRC."""
    _need_ref(ref)
    R = pkg.rx_binding
    sent = T.table_of(4, {(c, tn): (8 + (c + tn) % 3, 0) for c in range(4) for tn in (2, 4)})
    # c2's table names all four timeslots: the clock of a fresh receiver counts from 0, so its frames carry timeslots 1 and 3 -- they
    # would be routed if rule (b) did not hold them back
    table = [list(row) for row in sent]
    table[2][0], table[2][2] = (8, 0), (10, 0)
    cells = [(100 + 7 * c, 1000 + 13 * c, (5 + 3 * c) % 64) for c in range(4)]
    tx = [synth.gen_downlink(T.SLOTS, T.SEED + c, cell=cells[c], slot0=T.SLOT0, traffic={tn + 1: v for tn, v in enumerate(sent[c]) if v[0]})
          for c in range(4)]
    rng = np.random.default_rng(8)
    # c1: slot 33 (tn 2, frame 7) becomes a two-channel burst with the slot's own AACH
    stolen, code = 33, synth.tx_scramb_code(*cells[1])
    assert (stolen + T.SLOT0) % 4 + 1 == 2 and any(s == stolen for s, _, _ in tx[1][1]["tch"])
    ndb = rng.integers(0, 2, (2, 124), dtype=np.uint8)
    t5 = synth.tx_encode("ndb", ndb, [code, code])
    burst = tx[1][0][stolen * 510:(stolen + 1) * 510]
    bb = np.concatenate([burst[230:244], burst[266:282]])
    tx[1][0][stolen * 510:(stolen + 1) * 510] = synth.tx_norm_burst(t5[0], bb, t5[1], 1)
    # c2: the SB1 blocks of the first two SYNC bursts do not decode (the receiver locks on the first and reads the second)
    for s0 in (0, 4):
        tx[2][0][s0 * 510 + 94:s0 * 510 + 94 + 120] ^= rng.integers(0, 2, 120, dtype=np.uint8)
    iq = np.stack([synth.gen_channel(T.SAMPLES, T.SEED + 100 + c, bits=tx[c][0])[0] for c in range(4)])
    calls, drops, six, _, _ = _run(pkg, iq, table)
    got = _by_channel(_flat(calls))
    want = T.stream_rows(ref, oracle, iq, table, 0)
    assert got == want and sum(len(v) for v in got.values()) > 40
    rows = [r for k in got for r in got[k]]
    flat6 = {k: [r for c in six for r in c[k]] for k in range(R.N_KINDS)}
    # frame 18: SCH/F rows of the traffic timeslots exist there, TCH rows do not
    f18 = [r for r in flat6[R.KIND_SCH_F] if (r[4] >> 8) & 0xff == 18 and r[2]]
    assert len(f18) >= 6 and not [r for r in rows if (r[4] >> 8) & 0xff == 18]
    # the stolen slot
    s = stolen + T.SLOT0
    t_stolen = (s % 4 + 1) | ((s // 4) % 18 + 1) << 8 | ((s // 72) % 60 + 1) << 16
    assert not [r for r in rows if r[0] == 1 and r[4] == t_stolen] and len([r for r in rows if r[0] == 1]) >= 8
    for kind, pay in ((R.KIND_NDB1, ndb[0]), (R.KIND_NDB2, ndb[1])):
        assert [(r[2], r[5]) for r in flat6[kind] if r[0] == 1 and r[4] == t_stolen] == [(1, pay.tobytes())]
    # the fresh receiver: one-channel bursts before the first good SYNC PDU, none of them routed
    first_good = min(r[1] for r in flat6[R.KIND_SB1] if r[0] == 2 and r[2])
    first_any = min(r[1] for r in flat6[R.KIND_SB1] if r[0] == 2)
    early = [r for r in flat6[R.KIND_SCH_F] if r[0] == 2 and r[1] < first_good and 1 <= r[4] & 0xff <= 4 and (r[4] >> 8) & 0xff != 18]
    assert first_any < first_good and len(early) >= 2
    assert not [r for r in rows if r[0] == 2 and r[1] < first_good] and len([r for r in rows if r[0] == 2]) >= 4


@pytest.mark.parametrize("names", (("SOFT",), ("BITERR",), ("SOFT", "BITERR"), ("SOFT", "AACH_SOFT")), ids="_".join)
def test_gpu_traffic_under_the_create_flags(pkg, synth, oracle, ref, names):
    """The mixed table under TETRA_RX_FLAG_SOFT (TCH/4.8 and TCH/2.4 from the soft ring, TCH/7.2 from the packed frames still),
    _BITERR (the coded kinds' count words; refused for TCH/7.2), both, and SOFT | AACH_SOFT (the gate reads the maximum-likelihood row
    and its verdict): the matching definition's rows, labels and words."""
    _need_ref(ref)
    R = pkg.rx_binding
    flags = sum(getattr(R, "FLAG_" + n) for n in names)
    cells, tx, iq, _ = _mixed(synth, oracle)
    want = _want_mixed(ref, oracle, synth, flags)
    calls, drops, _, _, _ = _run(pkg, iq, T.MIXED, flags)
    got = _by_channel(_flat(calls))
    for k in T.TCH_KINDS:
        assert got[k] == want[k], (names, k, len(got[k]), len(want[k]))
        assert len(got[k]) >= 14 and all((r[6] is not None) == ("BITERR" in names and k in td.CODED) for r in got[k])
    T.assert_payloads(got, tx)
    if "SOFT" in names and "BITERR" not in names:       # the soft rows are not the hard ones' copies: the decoders saw other values
        assert _want_mixed(ref, oracle, synth, 0)[8] == want[8]


def test_gpu_traffic_leaves_the_six_kinds_unchanged(pkg, synth, oracle):
    """One stream, with traffic enabled and the mixed table versus never enabled (TETRA_RX_FLAG_BITERR, so that link figures exist):
    all six kinds' rows, verdicts and labels per call, the cell states and the link figures are identical."""
    R = pkg.rx_binding
    _, _, iq, _ = _mixed(synth, oracle)
    on = _run(pkg, iq, T.MIXED, R.FLAG_BITERR)
    off = _run(pkg, iq, T.MIXED, R.FLAG_BITERR, enable=False)
    assert on[2] == off[2] and sum(len(v) for c in on[2] for v in c.values()) > 300
    assert on[3] == off[3] and on[4] == off[4] and sum(l["blocks"] for l in on[4]) > 100
    assert sum(len(v) for v in _flat(on[0]).values()) == 43


def test_gpu_traffic_table_change_takes_effect_at_the_call_boundary(pkg, synth, oracle, ref):
    """The table changed right behind a call's enqueue, with that call and the one before it in flight: the call already enqueued is
    decoded with the table it was enqueued under, the next one with the new one.  Which call a frame belongs to is read off the calls'
    BBK rows, which the routing leaves alone."""
    _need_ref(ref)
    R = pkg.rx_binding
    cells, tx, iq, streams = _mixed(synth, oracle)
    other = T.table_of(4, {(0, 2): (9, 0), (1, 4): (8, 0), (2, 2): (10, 0), (3, 4): (8, 63), (3, 2): (10, 0)})
    k_change = len(CUTS) - 3                       # behind the last call but one
    calls, drops, six, _, _ = _run(pkg, iq, T.MIXED, change=(k_change, other))
    want = {name: T.stream_rows(ref, oracle, iq, table, 0, streams) for name, table in (("before", T.MIXED), ("after", other))}
    assert want["before"] != want["after"]
    n_before = n_after = 0
    for i, (c, s) in enumerate(zip(calls, six)):
        frames = {(r[0], r[1]) for r in s[R.KIND_BBK]}
        w = want["before" if i <= k_change else "after"]
        for k in T.TCH_KINDS:
            assert c[k] == [r for r in w[k] if (r[0], r[1]) in frames], (i, k)
            n_before, n_after = n_before + (len(c[k]) if i <= k_change else 0), n_after + (len(c[k]) if i > k_change else 0)
    assert n_before >= 10 and n_after >= 10, (n_before, n_after)
    # ... and the table reads back as it was set
    rx = pkg.RxChain(4, 1000)
    rx.enable_traffic(5)
    rx.set_traffic(T.table_arg(T.MIXED))
    rx.set_traffic(T.table_arg(other)[2:], first=2)
    t = rx.traffic()
    assert [[(int(e["kind"]), int(e["usage"])) for e in row] for row in t] == T.MIXED[:2] + other[2:] and not t["pad"].any()
    assert [[(int(e["kind"]), int(e["usage"])) for e in row] for row in rx.traffic(1, 2)] == [T.MIXED[1], other[2]]
    rx.close()


def test_gpu_traffic_overflow_keeps_the_first_rows(pkg, synth, oracle, ref):
    """max_rows = 3, the whole stream in one call: per kind the first three rows in (channel, frame) order, and n_dropped exact."""
    _need_ref(ref)
    cells, tx, iq, _ = _mixed(synth, oracle)
    want = _want_mixed(ref, oracle, synth, 0)
    calls, drops, _, _, _ = _run(pkg, iq, T.MIXED, cuts=[0, T.SAMPLES], max_samples=T.SAMPLES, max_rows=3)
    assert len(calls) == 1
    for k in T.TCH_KINDS:
        assert calls[0][k] == want[k][:3] and drops[0][k] == len(want[k]) - 3 > 0, k


def test_gpu_traffic_statuses(pkg, synth, oracle):
    """Before tetra_rx_traffic_enable every function is TETRA_ERR_UNSUPPORTED; the argument rules of each; no call yet: no rows."""
    import torch
    R = pkg.rx_binding
    L = R._lib()
    n, d = C.c_int(-1), C.c_int(-1)
    slot = np.zeros((1, 4), R.TRAFFIC_SLOT_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rx = pkg.RxChain(3, T.SAMPLES, flags=R.FLAG_BITERR)
    h = rx._h
    assert L.tetra_rx_set_traffic(h, 0, 1, p(slot), None) == UNSUPPORTED and L.tetra_rx_get_traffic(h, 0, 1, p(slot)) == UNSUPPORTED
    assert L.tetra_rx_fetch_traffic(h, 0, R.TCH_4_8, None, None, 0, 0, None, C.byref(n), None) == UNSUPPORTED
    assert L.tetra_rx_traffic_rows_device(h, 0, R.TCH_4_8, None, None, None, None, None, None) == UNSUPPORTED
    assert [L.tetra_rx_traffic_enable(h, m) for m in (0, -1, rx.max_rows + 1)] == [ARG] * 3
    assert L.tetra_rx_traffic_enable(h, rx.max_rows) == 0 and L.tetra_rx_traffic_enable(h, 1) == ARG
    assert not rx.traffic().view(np.uint8).any()                           # the table starts all zero
    for kind, usage in ((7, 0), (11, 0), (1, 0), (9, 1), (9, 3), (9, 64), (0, 255)):
        slot[0, 2]["kind"], slot[0, 2]["usage"] = kind, usage
        assert L.tetra_rx_set_traffic(h, 0, 1, p(slot), None) == ARG, (kind, usage)
    slot[0, 2]["kind"], slot[0, 2]["usage"] = 9, 4
    assert [L.tetra_rx_set_traffic(h, f, c, p(slot), None) for f, c in ((-1, 1), (3, 1), (0, -1), (2, 2))] == [ARG] * 4
    assert L.tetra_rx_set_traffic(h, 0, 1, None, None) == ARG and not rx.traffic().view(np.uint8).any()
    assert L.tetra_rx_set_traffic(h, 2, 1, p(slot), None) == 0 and L.tetra_rx_set_traffic(h, 3, 0, None, None) == 0
    assert rx.traffic(2, 1).tobytes() == bytes([0] * 8 + [9, 4, 0, 0] + [0] * 4)
    # no call yet
    assert L.tetra_rx_fetch_traffic(h, 0, R.TCH_4_8, None, None, 0, 0, None, C.byref(n), C.byref(d)) == 0 and (n.value, d.value) == (0, 0)
    assert L.tetra_rx_traffic_rows_device(h, 0, R.TCH_4_8, None, None, None, None, None, None) == ARG
    assert [L.tetra_rx_fetch_traffic(h, w, k, None, None, 0, c, None, C.byref(n), None) for w, k, c in ((2, 9, 0), (-1, 9, 0), (0, 7, 0), (0, 11, 0), (0, 9, -1))] == [ARG] * 5
    assert L.tetra_rx_fetch_traffic(h, 0, 9, None, None, 0, 0, None, None, None) == ARG
    _, _, iq, _ = _mixed(synth, oracle)
    rx.set_traffic(T.table_arg(T.MIXED[:3]))
    rx.process(iq[:3])
    blocks, t2, dropped, words = rx.fetch_traffic(R.TCH_4_8, biterr=True)
    m = len(blocks)
    assert m >= 10 and dropped == 0 and t2.shape == (m, 292) and (words >> 16 == 432).all() and (blocks["crc_ok"] == 1).all()
    buf = np.zeros((m, 292), np.uint8)
    assert L.tetra_rx_fetch_traffic(h, 0, 9, None, p(buf), 291, m, None, C.byref(n), None) == SIZE                 # stride below type 2
    assert L.tetra_rx_fetch_traffic(h, 0, 9, None, p(buf), 292, m - 1, None, C.byref(n), None) == SIZE and n.value == m
    assert L.tetra_rx_fetch_traffic(h, 0, 9, None, None, 0, 0, None, C.byref(n), None) == 0 and n.value == m       # one who only counts
    assert L.tetra_rx_fetch_traffic(h, 0, 8, None, None, 0, 0, p(buf), C.byref(n), None) == UNSUPPORTED            # TCH/7.2 is not coded
    wide = np.full((m, 300), 0xee, np.uint8)
    assert L.tetra_rx_fetch_traffic(h, 0, 9, None, p(wide), 300, m, None, C.byref(n), None) == 0
    assert np.array_equal(wide[:, :292], t2) and (wide[:, 292:] == 0xee).all()
    # the device view: the same rows where they lie
    dev_t2, stride, dev_blk, dev_cnt, dev_be = rx.traffic_rows_device(R.TCH_4_8, stream=torch.cuda.current_stream())
    assert stride == 296 and dev_be
    assert G.device_bytes(torch, dev_cnt, (3,), "<i4").cpu().numpy().tolist() == [m, m, 0]
    assert np.array_equal(G.device_bytes(torch, dev_t2, (m, 296), "|u1").cpu().numpy()[:, :292], t2)
    assert np.array_equal(G.device_bytes(torch, dev_be, (m,), "<u4").cpu().numpy(), words)
    assert rx.traffic_rows_device(R.TCH_7_2)[4] is None
    rx.close()
    plain = pkg.RxChain(2, 1000, kinds=1 << R.KIND_SCH_F)                   # no BBK rows: a gate has nothing to read, no flag: no words
    plain.enable_traffic()
    slot[0, 2]["usage"] = 4
    assert L.tetra_rx_set_traffic(plain._h, 0, 1, p(slot), None) == ARG
    slot[0, 2]["usage"] = 0
    assert L.tetra_rx_set_traffic(plain._h, 0, 1, p(slot), None) == 0
    assert L.tetra_rx_fetch_traffic(plain._h, 0, 9, None, None, 0, 0, p(buf), C.byref(n), None) == UNSUPPORTED
    plain.close()


def _wide_capture(torch, synth, M, carriers, traffic, nslots):
    """tests/wideband_gpu.capture with a traffic option per carrier: {bin: seed} -> (x complex64 [n] on cuda, tx {bin: gen_downlink})"""
    dev = torch.device("cuda")
    N = (nslots * 510 - 100) // 9 * 9
    Ln = int(round(N * M * 25000.0 / 36000.0))
    x = torch.zeros(Ln, dtype=torch.complex128, device=dev)
    n = torch.arange(Ln, dtype=torch.float64, device=dev)
    tx = {}
    for k, sd in carriers.items():
        tx[k] = synth.gen_downlink(nslots, sd, cell=(100 + 7 * sd % 900, 1000 + 13 * sd, (5 + 3 * sd) % 64), traffic=traffic.get(k),
                                   aach_codewords=T.codewords())
        s = torch.from_numpy(synth.gen_channel(N, sd + 100, bits=tx[k][0], amp=1.0)[0].astype(np.complex128)).to(dev)
        S = torch.fft.fft(s)
        Y = torch.zeros(Ln, dtype=torch.complex128, device=dev)
        Y[: N // 2] = S[: N // 2]
        Y[Ln - (N - N // 2):] = S[N // 2:]
        kc = k if k < M // 2 else k - M
        x += torch.fft.ifft(Y) * (Ln / N) * torch.polar(torch.ones_like(n), 2.0 * math.pi * kc / M * n)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x += 1e-3 * torch.view_as_complex(torch.randn((Ln, 2), device=dev, generator=g, dtype=torch.float64))
    x *= 0.25 / float(x.abs().max())
    return x.to(torch.complex64).contiguous(), tx


def test_gpu_traffic_through_the_wideband_receiver(pkg, synth):
    """A small WidebandRx (32 bins, 3 carriers), one call: the carrier slot whose table entries name its traffic timeslots returns one
    TCH row for every one-channel burst the chain found in those timeslots behind the carrier's first good SYNC PDU (the SCH/F rows of
    the same call say which) and no other; from slot 28 on (tests/test_wbrx.py's settling rule) every row carries the payload sent in
    the slot its TDMA time names; the other carriers return none.  The capture holds 16 traffic slots from slot 28 on; the loops may
    still drop a frame there, so at least half of them must come back."""
    import torch
    R = pkg.rx_binding
    bins, nslots = [1, 7, 20], 60
    traffic = {7: {2: (R.TCH_2_4, 21), 4: (R.TCH_4_8, 0)}}
    x, tx = _wide_capture(torch, synth, 32, {1: 11, 7: 12, 20: 13}, traffic, nslots)
    wb = pkg.WidebandRx(bins, n_channels=32, decimation=16, max_in=x.shape[0])
    wb.enable_traffic()
    wb.set_traffic([None, traffic[7], None])
    assert [[int(e["kind"]) for e in row] for row in wb.traffic()] == [[0] * 4, [0, R.TCH_2_4, 0, R.TCH_4_8], [0] * 4]
    wb.process_device(x, x.shape[0])
    sent = {}
    for slot, kind, pay in tx[7][1]["tch"]:
        tn, fn, mn = synth.tdma_time_of_slot(slot)
        sent[tn | fn << 8 | mn << 16] = (slot, kind, pay)
    six = G.collect(wb.rx, R)
    first_good = min(r[1] for r in six[R.KIND_SB1] if r[0] == 1 and r[2])
    frames = {tn: sorted((r[1], r[4]) for r in six[R.KIND_SCH_F] if r[0] == 1 and r[1] > first_good and r[4] & 0xff == tn) for tn in (2, 4)}
    exact = 0
    for k, tn in ((R.TCH_2_4, 2), (R.TCH_4_8, 4), (R.TCH_7_2, 0)):
        blocks, t2, dropped = wb.fetch_traffic(k)
        assert dropped == 0 and (blocks["channel"] == 1).all()
        assert [(int(b["bitnum"]), int(b["tdma_time"])) for b in blocks] == frames.get(tn, []), k
        for b, row in zip(blocks, t2):
            if b["bitnum"] < 28 * 510:
                continue
            slot, kind, pay = sent[int(b["tdma_time"])]
            assert kind == k and np.array_equal(row[:len(pay)], pay), (k, slot)
            exact += 1
    assert exact >= 8, exact
    wb.close()
    torch.cuda.synchronize()


def test_gpu_traffic_host_banks(pkg, synth, oracle, tmp_path):
    """TetraRxBank::enableTraffic / setTraffic / fetchTraffic and the TetraRxMultiBank forms (host/tetra_rx_bank.h), 2 shards on one GPU,
    on the mixed table's stream in one call: the shards' rows one after the other are the single bank's, in the bank's channel numbers,
    and as many per kind as the definition routes (tests/test_rx_traffic.py pins the counts to it).  A plain C++ driver
    (tests/host/test_traffic_bank.cpp)."""
    from tests.restart_gpu import build_and_run_bank_driver
    R = pkg.rx_binding
    _, _, iq, _ = _mixed(synth, oracle)
    f_iq, f_table = str(tmp_path / "iq.bin"), str(tmp_path / "table.bin")
    np.ascontiguousarray(iq).tofile(f_iq)
    R.traffic_table_arg(T.table_arg(T.MIXED)).tofile(f_table)
    r = build_and_run_bank_driver(pkg, "test_traffic_bank", [T.CHANNELS, 2, T.SAMPLES, f_iq, f_table])
    assert r.returncode == 0 and "test_traffic_bank: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert [line.split()[1:] for line in r.stdout.splitlines() if line.startswith("rows ")] == [["8", "14"], ["9", "14"], ["10", "15"]]
