"""Training-sequence search against the REFERENCE ITSELF: oracle/_ref is the reference's
phy/tetra_burst.c compiled from /root/reference (oracle/build_ref.sh), so parity for this entry point is pinned."""
import numpy as np
import pytest

SEQS = None


def _seqs():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "etsi_training_sequences.json")) as f:
        ts = json.load(f)
    return {0: ts["normal_1"], 1: ts["normal_2"], 2: ts["normal_3"], 3: ts["sync"], 4: ts["extended"]}


def test_reference_library_finds_its_own_training_sequences(ref):
    seqs = _seqs()
    for t, s in seqs.items():
        row = np.zeros(600, np.uint8)
        row[100:100 + len(s)] = s
        assert ref.find_train_seq(row, 510) == (t, 100)
    rng = np.random.default_rng(0)
    nb = ref.build_norm_burst(rng.integers(0, 2, 216), rng.integers(0, 2, 30), rng.integers(0, 2, 216), 0)
    sb = ref.build_sync_burst(rng.integers(0, 2, 120), rng.integers(0, 2, 30), rng.integers(0, 2, 216))
    assert nb.size == 510 and sb.size == 510
    assert ref.find_train_seq(np.concatenate([nb, np.zeros(64, np.uint8)]), 510) == (ref.TRAIN_NORM_1, 244)
    assert ref.find_train_seq(np.concatenate([sb, np.zeros(64, np.uint8)]), 510) == (ref.TRAIN_SYNC, 214)


def test_reference_lookahead_quirk_exists(ref):
    """The reference's pre-filter skips in[20] for the first 21 positions: a sequence at position 3 is missed,
    the same sequence at position 30 is found (documented in include/tetra_burst_scan.h and reproduced on the GPU)."""
    s = _seqs()[0]
    row = np.zeros(200, np.uint8)
    row[3:3 + 22] = s
    early = ref.find_train_seq(row, 150)
    row2 = np.zeros(200, np.uint8)
    row2[30:30 + 22] = s
    assert ref.find_train_seq(row2, 150) == (0, 30)
    assert early != (0, 3)


@pytest.mark.gpu
def test_gpu_scan_equals_reference_on_planted_and_random_rows(pkg, ref):
    seqs = _seqs()
    rng = np.random.default_rng(42)
    Cn, stride = 600, 20000 + 64
    rows = rng.integers(0, 2, (Cn, stride), dtype=np.uint8)
    end = rng.integers(1, 20000, Cn).astype(np.int32)
    end[:40] = np.arange(1, 41)                       # tiny rows
    end[40:80] = 20000                                # full rows (one tile: a tile is 32768 positions; the tests at the end of this file cross it)
    for c in range(Cn):
        k = rng.integers(0, 4)
        for _ in range(k):
            t = int(rng.integers(0, 5))
            pos = int(rng.choice([rng.integers(0, 48), rng.integers(0, max(1, end[c])), max(0, end[c] - rng.integers(0, 45))]))
            s = seqs[t]
            if pos + len(s) <= stride:
                rows[c, pos:pos + len(s)] = s
    rows[100:130] = 0                                 # rows with nothing in them
    for mask in (0x1f, 0x08, 0x07, 0x10, 0x01):
        tg, og = pkg.scan_binding.find_train_seq_batch(rows, end, mask)
        for c in range(Cn):
            assert (int(tg[c]), int(og[c])) == ref.find_train_seq(rows[c], int(end[c]), mask), (c, mask, end[c])


@pytest.mark.gpu
def test_reference_bursts_through_the_gpu_demodulator(pkg, ref, synth):
    """Reference-built known answer for the whole path: continuous downlink bursts from the reference's own builders
    (tetra_burst.c:171-269) -> pi/4-DQPSK IQ -> GPU demodulator -> the reference's own tetra_find_train_seq locks onto
    the output at 510-bit slot spacing, and the GPU scan reports the same (type, offset) pairs."""
    rng = np.random.default_rng(7)
    Cn, nslots = 12, 40
    tx = []
    for c in range(Cn):
        slots = []
        for s in range(nslots):
            if s % 4 == 0:
                slots.append(ref.build_sync_burst(rng.integers(0, 2, 120), rng.integers(0, 2, 30), rng.integers(0, 2, 216)))
            else:
                slots.append(ref.build_norm_burst(rng.integers(0, 2, 216), rng.integers(0, 2, 30), rng.integers(0, 2, 216), s % 2))
        tx.append(np.concatenate(slots))
    N = nslots * 510 - 200
    iq = np.stack([synth.gen_channel(N, 300 + c, bits=tx[c])[0] for c in range(Cn)])
    d = pkg.Demodulator(Cn, N)
    bits, nb, _ = d.process(iq)
    d.close()
    # walk every channel with the reference finder, restarting after each hit, and with the GPU finder on the same rows
    for c in range(Cn):
        hits = []
        pos = 6000
        while pos < nb[c] - 600:
            t, o = ref.find_train_seq(bits[c][pos:], int(nb[c] - pos - 64))
            if t < 0:
                break
            hits.append((t, pos + o))
            pos += o + 60
        assert len(hits) >= 25, (c, hits[:5])
        sync_hits = [o for t, o in hits if t == ref.TRAIN_SYNC]
        assert len(sync_hits) >= 5 and all((b - a) % (4 * 510) == 0 for a, b in zip(sync_hits, sync_hits[1:]))
        norm_hits = [o for t, o in hits if t in (ref.TRAIN_NORM_1, ref.TRAIN_NORM_2)]
        assert all((b - a) % 510 == 0 for a, b in zip(norm_hits, norm_hits[1:]))
    # batched GPU scan of the tail of every channel == reference
    start = 8000
    sub = np.ascontiguousarray(bits[:, start:start + 4096 + 64])
    end = np.full(Cn, 4096, np.int32)
    tg, og = pkg.scan_binding.find_train_seq_batch(sub, end)
    for c in range(Cn):
        assert (int(tg[c]), int(og[c])) == ref.find_train_seq(sub[c], 4096), c


# ---------------------------------------------------------------------------------------------------------------------
# The plugin's own training-sequence indicator (src/main.cpp:385-414)
# ---------------------------------------------------------------------------------------------------------------------
IND_SEQS = {
    "n": [1,1, 0,1, 0,0, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,1, 0,0],
    "p": [0,1, 1,1, 1,0, 1,0, 0,1, 0,0, 0,0, 1,1, 0,1, 1,1, 1,0],
    "q": [1,0, 1,1, 0,1, 1,1, 0,0, 0,0, 0,1, 1,0, 1,0, 1,1, 0,1],
    "N": [1,1,1, 0,0,1, 1,0,1, 1,1,1, 0,0,0, 1,1,1, 1,0,0, 0,1,1, 1,1,0, 0,0,0, 0,0,0],
    "P": [1,0,1, 0,1,1, 1,1,1, 1,0,1, 0,1,0, 1,0,1, 1,1,0, 0,0,1, 1,0,0, 0,1,0, 0,1,0],
    "x": [1,0, 0,1, 1,1, 0,1, 0,0, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,1, 0,0, 0,0, 1,1],
    "X": [0,1,1,1,0,0,1,1,0,1,0,0,0,0,1,0,0,0,1,1,1,0,1,1,0,1,0,1,0,1,1,1,1,1,0,1,0,0,0,0,0,1,1,1,0],
    "y": [1,1, 0,0, 0,0, 0,1, 1,0, 0,1, 1,1, 0,0, 1,1, 1,0, 1,0, 0,1, 1,1, 0,0, 0,0, 0,1, 1,0, 0,1, 1,1],
}


def test_indicator_restatement_arms_and_expires(oracle):
    """Known answers worked out by hand from main.cpp:385-414: a sequence of length L that ends at bit e is seen when the
    window's head holds it, 45 - L bits later; that bit arms 2048 and counts it down to 2047; 2047 further bits clear it."""
    for name, seq in IND_SEQS.items():
        L = len(seq)
        o = oracle.TsIndicatorOracle()
        pre = np.zeros(100, np.uint8)
        assert o.feed(pre) == (False, 0)
        assert o.feed(np.array(seq, np.uint8)) == ((True, 2047) if L == 45 else (False, 0)), name
        if L < 45:
            assert o.feed(np.zeros(45 - L - 1, np.uint8)) == (False, 0), name
            assert o.feed(np.zeros(1, np.uint8)) == (True, 2047), name
        again = 4 if name == "x" else 0        # the extended sequence holds normal sequence 1 at its bit 4: a second hit re-arms
        assert o.feed(np.zeros(2046, np.uint8)) == (True, 1 + again), name
        assert o.feed(np.zeros(again, np.uint8)) == (True, 1), name
        assert o.feed(np.zeros(1, np.uint8)) == (False, 0), name
    # the ETSI sequences of the fixture are the plugin's n / p / q / y / x
    ts = _seqs()
    assert ts[0] == IND_SEQS["n"] and ts[1] == IND_SEQS["p"] and ts[2] == IND_SEQS["q"] and ts[3] == IND_SEQS["y"] and ts[4] == IND_SEQS["x"]


@pytest.mark.gpu
def test_gpu_indicator_equals_the_restatement_chunked_with_carried_state(pkg, oracle):
    """600 channels of random bits with planted sequences (also across call boundaries and inside the first 44 bits of a
    call), ragged per-channel counts and call lengths from 0 to several tiles: tsfound and symsbeforeexpire after every call
    equal the literal restatement's; reset of one channel and of all."""
    rng = np.random.default_rng(7)
    Cn, total = 600, 60000
    rows = rng.integers(0, 2, (Cn, total), dtype=np.uint8)
    rows[:20] = 0                                           # quiet channels: only planted hits
    names = list(IND_SEQS)
    for c in range(Cn):
        for _ in range(int(rng.integers(0, 5))):
            s = IND_SEQS[names[int(rng.integers(0, 8))]]
            pos = int(rng.integers(0, total - 64))
            rows[c, pos:pos + len(s)] = s
    ind = pkg.scan_binding.TsIndicator(Cn)
    orcs = [oracle.TsIndicatorOracle() for _ in range(Cn)]
    pos = np.zeros(Cn, np.int64)
    for k, base_len in enumerate([1, 43, 44, 45, 0, 300, 2047, 2048, 2049, 9000, 17000, 8192, 31]):
        nb = np.minimum(base_len + (rng.integers(0, 40, Cn) if k % 2 else 0), total - pos).astype(np.int32)
        if base_len == 0:
            nb[:] = 0
        stride = (int(nb.max()) + 8 + 3) & ~3
        bits = np.zeros((Cn, stride), np.uint8)
        for c in range(Cn):
            bits[c, :nb[c]] = rows[c, pos[c]:pos[c] + nb[c]]
        found, expire = ind.process(bits, nb)
        for c in range(Cn):
            want = orcs[c].feed(rows[c, pos[c]:pos[c] + nb[c]])
            assert (bool(found[c]), int(expire[c])) == want, (k, c, base_len)
        pos += nb
        if k == 6:
            ind.reset(3)
            orcs[3] = oracle.TsIndicatorOracle()
    assert found[20:].any() and not found[20:].all()
    ind.reset()
    f, e = ind.process(np.zeros((Cn, 8), np.uint8), np.zeros(Cn, np.int32))
    assert not f.any() and not e.any()
    with pytest.raises(pkg.TetraDemodError):
        ind.reset(Cn)
    ind.close()


@pytest.mark.gpu
def test_gpu_indicator_sees_the_demodulated_downlink(pkg, synth):
    """End of the chain the plugin runs in NETSYMS mode: synthetic downlink bursts -> demodulator -> indicator: found on the
    burst channels, not on noise."""
    import torch
    Cn, N = 6, 36000
    iq = np.zeros((Cn, N), np.complex64)
    for c in range(Cn - 1):
        iq[c] = synth.gen_channel(N, 100 + c, bits=synth.gen_slot_bits(N // 510 + 2, 100 + c))[0]
    rng = np.random.default_rng(5)
    iq[Cn - 1] = (0.3 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    d = pkg.Demodulator(Cn, N)
    bits, nb, _ = d.process(iq)
    ind = pkg.scan_binding.TsIndicator(Cn)
    found, expire = ind.process(bits, nb)
    assert found[:Cn - 1].all() and not found[Cn - 1], (found, expire)
    ind.close()
    d.close()


# ---------------------------------------------------------------------------------------------------------------------
# Tile edges, packing routes, clamps and the device entries.  The cases below are shared: the CPU tests run them through the
# host build of the kernels' own lane code (tests/emul/scan_emul.cpp = csrc/scan_core.hpp) against the reference's function,
# and pin the restated search to the reference on the same long rows; the GPU tests run them through the kernels against that
# restatement (oracle/_ref does not travel with a checkout, the restatement does).
# ---------------------------------------------------------------------------------------------------------------------
TILE = 32768          # scan_core::kTile
IND_TILE = 8192       # scan_core::kIndTile
ALL = 0x1f
LENGTHS = (32767, 32768, 32769, 32768 + 21, 32768 + 22, 36000, 65536 + 100, 100000)
ROUTE_STRIDES = (36032, 36036, 36056, 36060, 36048)     # % 16 = 0, 4, 8, 12, 0; % 32 = 24 and 28 put bits below end_of_in into the byte route
_CASES, _WANT = {}, {}


@pytest.fixture(scope="module")
def scan_emul():
    from tests.emul import scan_emul_bind
    scan_emul_bind.build()
    assert scan_emul_bind.tile() == TILE and scan_emul_bind.ind_tile() == IND_TILE
    return scan_emul_bind


def _quiet(stride, *plants):
    row = np.zeros(stride, np.uint8)
    seqs = _seqs()
    for t, p in plants:
        row[p:p + len(seqs[t])] = seqs[t]
    return row


def _case_edge(edge):
    """Each sequence at every position from 38 before a tile edge to 1 past it, once with end_of_in one short of the sequence's
    last bit and once just holding it: the last position of a tile (shift 31), the first of the next, every way a 22-, 30- or
    38-bit sequence lies across the edge."""
    seqs, stride = _seqs(), edge + 128
    rows, end = [], []
    for t in range(5):
        for p in range(edge - 38, edge + 2):
            for e in (p + len(seqs[t]) - 1, p + len(seqs[t])):
                rows.append(_quiet(stride, (t, p)))
                end.append(e)
    return np.stack(rows), np.array(end, np.int32), (ALL,)


def _case_lengths():
    """Per row length: each sequence ending exactly at end_of_in and one bit past it, an empty row and a random one."""
    seqs, stride = _seqs(), 100000 + 64
    rng = np.random.default_rng(11)
    rows, end = [], []
    for n in LENGTHS:
        for t in range(5):
            for p in (n - len(seqs[t]), n - len(seqs[t]) + 1):
                rows.append(_quiet(stride, (t, p)))
        rows.append(_quiet(stride))
        rows.append(rng.integers(0, 2, stride, dtype=np.uint8))
        end += [n] * 12
    return np.stack(rows), np.array(end, np.int32), (ALL,)


def _case_order():
    """Early exit and check order across tiles, under every single-sequence mask and every mask with one sequence taken out."""
    stride, n = 100000 + 64, 100000
    SY, N1, N2, N3, EX = 3, 0, 1, 2, 4
    rows = [
        _quiet(stride, (N1, 5000), (SY, 40000)),               # tile 0's hit wins over an earlier check order in tile 1
        _quiet(stride, (SY, 70000)),                           # a hit only in tile 2
        _quiet(stride, (N1, 40000), (SY, 41000)),              # two hits in one tile
        _quiet(stride, (N3, 45000), (N1, 44000)),
        _quiet(stride, (SY, TILE - 10), (N1, 100)),            # with normal 1 masked out the answer lies across the edge
        _quiet(stride, (EX, 2 * TILE - 3), (N2, 3 * TILE - 1), (N3, 3 * TILE + 9)),
    ]
    at = (1000, 33000, 50000, 66000, 99000)                    # tiles 0, 1, 1, 2, 3: the five sequences in every rotation
    for k in range(5):
        rows.append(_quiet(stride, *[((j + k) % 5, at[j]) for j in range(5)]))
    masks = (ALL, 0) + tuple(1 << t for t in range(5)) + tuple(ALL ^ (1 << t) for t in range(5))
    return np.stack(rows), np.full(len(rows), n, np.int32), masks


def _case_route(stride):
    """One batch per stride: with stride % 16 != 0 its rows lie at every 4-byte alignment in turn."""
    rng = np.random.default_rng(stride)
    SY, N1, EX = 3, 0, 4
    rows = [rng.integers(0, 2, stride, dtype=np.uint8), _quiet(stride, (SY, TILE - 20)), _quiet(stride, (N1, stride - 43)),
            _quiet(stride, (EX, 100), (SY, 20))]
    end = [36000, 36000, stride - 21, 36000]
    for e in (stride - 21, 36000, 33000, TILE):
        row = rng.integers(0, 2, stride, dtype=np.uint8)
        row[: e - 3000] = 0
        for t in range(5):
            p = int(rng.integers(e - 3000, e - 38))
            row[p:p + len(_seqs()[t])] = _seqs()[t]
        rows.append(row)
        end.append(e)
    return np.stack(rows), np.array(end, np.int32), (ALL, 1 << SY)


def _case_clamp(stride):
    """end_of_in at and past bits_stride, zero and negative; sequences reaching into the last 21 bytes of a row, lying across two
    rows and opening the next row: a count that is not cut back finds them."""
    SY, N1, N2, EX = 3, 0, 1, 4
    rows = np.stack([
        _quiet(stride, (N1, stride - 30)),                     # reaches into the row's last 21 bytes: outside the cut-back count
        _quiet(stride, (N1, stride - 21 - 22)),                # ends exactly where the cut-back count ends: found
        _quiet(stride, (N2, stride - 21 - 21)),                # one bit past it; the next row opens with a sequence
        _quiet(stride, (N1, 0), (SY, 100)),
        _quiet(stride, (SY, 100)),
        _quiet(stride, (EX, stride - 21 - 30)),
    ])
    y = _seqs()[SY]
    flat = rows.reshape(-1)
    flat[stride - 10: stride - 10 + 38] = y                    # a sync sequence across rows 0 and 1
    flat[5 * stride - 6: 5 * stride - 6 + 38] = y              # and across rows 4 and 5
    end = np.array([stride, stride + 1000, stride + 1000, 0, -5, stride], np.int32)
    return rows, end, (ALL,)


def _case(name):
    if name not in _CASES:
        kind, _, arg = name.partition(":")
        make = {"edge": _case_edge, "lengths": _case_lengths, "order": _case_order, "route": _case_route, "clamp": _case_clamp}[kind]
        rows, end, masks = make(int(arg)) if arg else make()
        _CASES[name] = (rows, end, masks)
    return _CASES[name]


SEARCH_CASES = ["edge:%d" % TILE, "edge:%d" % (2 * TILE), "lengths", "order", "clamp:4160", "clamp:%d" % (TILE + 64)] + \
               ["route:%d" % s for s in ROUTE_STRIDES]


def _want(judge, name, mask):
    """What `judge` (the reference's function or its restatement, one row at a time) says about a case: the documented cut-back of
    end_of_in to bits_stride - 21 applied first, and (-1, -1) for a count that is not positive.  Computed once per process."""
    key = (judge, name, mask)
    if key not in _WANT:
        rows, end, _ = _case(name)
        out = []
        for c in range(rows.shape[0]):
            e = min(int(end[c]), rows.shape[1] - 21)
            out.append(judge(rows[c], e, mask) if e > 0 else (-1, -1))
        _WANT[key] = out
    return _WANT[key]


def _pairs(t, o):
    return [(int(a), int(b)) for a, b in zip(t, o)]


@pytest.mark.parametrize("name", SEARCH_CASES)
def test_restated_search_equals_reference_on_long_rows(ref, oracle, name):
    """The restatement has no length limit of its own (unsigned counters like the reference's): pinned here on rows of 32767 to
    100000 bits, so that the GPU tests below can use it where oracle/_ref is absent."""
    for mask in _case(name)[2]:
        assert _want(oracle.bsync_find_train_seq, name, mask) == _want(ref.find_train_seq, name, mask), mask


def test_search_cases_hold_what_they_claim(ref):
    """The reference on the planted rows: a sequence that just fits is found where it was planted, one that is a bit short is not."""
    seqs = _seqs()
    for edge in (TILE, 2 * TILE):
        want = _want(ref.find_train_seq, "edge:%d" % edge, ALL)
        k = 0
        for t in range(5):
            for p in range(edge - 38, edge + 2):
                assert want[k] != (t, p) and want[k + 1] == (t, p), (edge, t, p)
                k += 2
    want = _want(ref.find_train_seq, "lengths", ALL)
    for i, n in enumerate(LENGTHS):
        for t in range(5):
            assert want[12 * i + 2 * t] == (t, n - len(seqs[t])) and want[12 * i + 2 * t + 1] != (t, n - len(seqs[t]) + 1)
        assert want[12 * i + 10] == (-1, -1)
    want = _want(ref.find_train_seq, "order", ALL)
    assert want[:4] == [(0, 5000), (3, 70000), (0, 40000), (0, 44000)]
    assert _want(ref.find_train_seq, "order", ALL ^ 1)[4] == (3, TILE - 10)
    for stride in (4160, TILE + 64):
        assert _want(ref.find_train_seq, "clamp:%d" % stride, ALL) == [(-1, -1), (0, stride - 43), (-1, -1), (-1, -1), (-1, -1), (4, stride - 51)]


@pytest.mark.parametrize("name", SEARCH_CASES)
def test_emulated_scan_equals_reference(ref, scan_emul, name):
    """The kernel's lane code, walked as a workgroup walks a row, on every case; the early exit packs exactly the tiles up to the one
    that holds the answer; no load that the hardware could not make.
    (The exit before the tile at `base` asks for a match at a position < base.  `<=` would do the same on every input: matches of
    earlier tiles lie below base, and before tile 0 only the pre-filter has run, which cannot match at position 0 -- its filter
    holds 21 bits there, so only normal sequence 2's head, the one with a leading 0, can equal it, which asks for in[0..19] =
    p[1..20] = 1,1,1,1,0,..., and no sequence begins like that.)"""
    rows, end, masks = _case(name)
    scan_emul.trace()
    for mask in masks:
        t, o, tiles = scan_emul.find_train_seq_batch(scan_emul.rows_at(rows), end, mask)
        want = _want(ref.find_train_seq, name, mask)
        assert _pairs(t, o) == want, mask
        for c, (_, off) in enumerate(want):
            e = min(int(end[c]), rows.shape[1] - 21)
            assert tiles[c] == ((off // TILE + 1) if off >= 0 else max(0, -(-e // TILE))), (c, mask)
    assert scan_emul.trace()["misaligned"] == 0


@pytest.mark.parametrize("stride", ROUTE_STRIDES)
def test_emulated_scan_takes_every_packing_route(ref, scan_emul, stride):
    """The same rows at every 4-byte alignment of the base: the answers do not change, 16-byte loads are made exactly where the
    address allows them, and a stride that is a multiple of 16 says nothing about a base that is not."""
    name = "route:%d" % stride
    rows, end, masks = _case(name)
    for offset in (0, 4, 8, 12):
        for mask in masks:
            scan_emul.trace()
            t, o, _ = scan_emul.find_train_seq_batch(scan_emul.rows_at(rows, offset), end, mask)
            tr = scan_emul.trace()
            assert _pairs(t, o) == _want(ref.find_train_seq, name, mask), (offset, mask)
            assert tr["misaligned"] == 0 and tr["route1"] > 0, (offset, tr)
            aligned = [(offset + c * stride) % 16 == 0 for c in range(rows.shape[0])]
            assert (tr["route16"] > 0, tr["route4"] > 0) == (any(aligned), not all(aligned)), (offset, tr)


# ---- the indicator ---------------------------------------------------------------------------------------------------
def _indicator_schedule():
    """Channels x calls for the window across a tile or word edge.  Per sequence and per q -- the call bit on which the sequence's last
    bit falls: 8191 - 44 .. 8192 + 1, the same around 16384, and the last 33 bits of a call, where the packer leaves the dword route --
    two channels with the same stream: one takes it in one call, the other has the call boundary inside the sequence.  Then 2000 and
    100 quiet bits, over which the counters run out.  -> list of calls, each (bits uint8 [C][stride], n_bits int32 [C])."""
    if "ind" in _CASES:
        return _CASES["ind"]
    streams, first = [], []
    for seq in IND_SEQS.values():
        L = len(seq)
        plan = [(q, IND_TILE + 64) for q in range(IND_TILE - 1 - 44, IND_TILE + 2)]
        plan += [(q, 2 * IND_TILE + 64) for q in range(2 * IND_TILE - 1 - 44, 2 * IND_TILE + 2)]
        plan += [(q, 300) for q in range(300 - 33, 300)]
        for q, n in plan:
            s = np.zeros(n, np.uint8)
            s[q - L + 1:q + 1] = seq
            streams += [s, s]
            first += [n, q + 1 - (1 + q % (L - 1))]           # whole, or cut 1 .. L - 1 bits before the sequence's end
    Cn, stride = len(streams), 2 * IND_TILE + 64
    calls = []
    for k in range(2):
        bits, nb = np.zeros((Cn, stride), np.uint8), np.zeros(Cn, np.int32)
        for c, s in enumerate(streams):
            part = s[:first[c]] if k == 0 else s[first[c]:]
            bits[c, :part.size] = part
            nb[c] = part.size
        calls.append((bits, nb))
    calls.append((np.zeros((Cn, 2000), np.uint8), np.full(Cn, 2000, np.int32)))
    calls.append((np.zeros((Cn, 100), np.uint8), np.full(Cn, 100, np.int32)))
    _CASES["ind"] = calls
    return calls


def _indicator_want(oracle):
    """The literal restatement's (found, expire) after every call of the schedule, computed once per process."""
    if "ind" not in _WANT:
        calls = _indicator_schedule()
        orcs = [oracle.TsIndicatorOracle() for _ in range(calls[0][0].shape[0])]
        _WANT["ind"] = [[o.feed(bits[c, :nb[c]]) for c, o in enumerate(orcs)] for bits, nb in calls]
        first = _WANT["ind"]
        assert any(f for f, _ in first[0]) and any(f for f, _ in first[1]) and any(f for f, _ in first[2]) and not any(f for f, _ in first[3])
    return _WANT["ind"]


def _check_indicator(ind, want, calls=None):
    for k, (bits, nb) in enumerate(calls or _indicator_schedule()):
        found, expire = ind.process(bits, nb)
        got = [(bool(f), int(e)) for f, e in zip(found, expire)]
        bad = [c for c in range(len(got)) if got[c] != want[k][c]]
        assert not bad, (k, bad[:5], [got[c] for c in bad[:5]], [want[k][c] for c in bad[:5]])


def test_emulated_indicator_equals_the_restatement_across_tile_and_call_edges(oracle, scan_emul):
    scan_emul.trace()
    _check_indicator(scan_emul.TsIndicator(_indicator_schedule()[0][0].shape[0]), _indicator_want(oracle))
    tr = scan_emul.trace()
    assert tr["misaligned"] == 0 and tr["route4"] > 0 and tr["route1"] > 0


def _clamp_calls(oracle, stride=512):
    """Calls for the indicator's clamps, with what the restatement says after each: a negative count is a count of 0 (state untouched,
    outputs from the carried counter), a count past the stride is the stride."""
    rng = np.random.default_rng(3)
    Cn = 4
    x = IND_SEQS["x"]
    a = rng.integers(0, 2, (Cn, stride), dtype=np.uint8)
    a[:, 60:60 + 30] = x
    a[1, stride - 20:] = x[:20]                               # the sequence's other 10 bits open the next call
    b = rng.integers(0, 2, (Cn, stride), dtype=np.uint8)
    b[1, :10] = x[20:]
    na = np.array([200, stride + 100, 300, 0], np.int32)
    calls = [(a, na), (b, np.full(Cn, -3, np.int32)), (b, np.array([50, 50, stride + 100, -1], np.int32))]
    orcs = [oracle.TsIndicatorOracle() for _ in range(Cn)]
    want = []
    for bits, nb in calls:
        want.append([o.feed(bits[c, :min(max(int(nb[c]), 0), stride)]) for c, o in enumerate(orcs)])
    assert want[0] == want[1] and want[0][0][0] and want[2][1][0] and want[2][1][1] > 2047 - 50      # armed by the split sequence
    return calls, want


def test_emulated_indicator_clamps_its_counts(oracle, scan_emul):
    calls, want = _clamp_calls(oracle)
    _check_indicator(scan_emul.TsIndicator(4), want, calls)


# ---- the kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SEARCH_CASES)
def test_gpu_scan_equals_the_pinned_restatement_across_tiles(pkg, oracle, name):
    """Every case above through k_find_train_seq (host entry): rows longer than one, two and three tiles, sequences across the
    tile edges, the early exit, the masks, the three packing routes by stride and the cut-back of end_of_in."""
    rows, end, masks = _case(name)
    for mask in masks:
        t, o = pkg.scan_binding.find_train_seq_batch(rows, end, mask)
        assert _pairs(t, o) == _want(oracle.bsync_find_train_seq, name, mask), mask


def _device_find(pkg, rows, end, mask, offset=0, stream=None):
    """tetra_find_train_seq_batch_device on a side stream, the rows `offset` bytes into a torch buffer between guard bytes of 1."""
    import torch
    dev = torch.device("cuda", 0)
    Cn, stride = rows.shape
    guard, used = 64, Cn * stride
    buf = torch.ones(guard + offset + used + guard, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    buf[guard + offset: guard + offset + used] = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).to(dev)
    d_end = torch.from_numpy(np.ascontiguousarray(end, np.int32)).to(dev)
    t = torch.full((Cn,), -7, dtype=torch.int32, device=dev)
    o = torch.full((Cn,), -7, dtype=torch.int32, device=dev)
    s = stream or torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    pkg.scan_binding.find_train_seq_batch_device(buf.data_ptr() + guard + offset, Cn, stride, d_end, mask, t, o, s)
    s.synchronize()
    assert bool((buf[:guard + offset] == 1).all()) and bool((buf[guard + offset + used:] == 1).all())
    return t.cpu().numpy(), o.cpu().numpy()


@pytest.mark.gpu
def test_gpu_scan_device_entry_on_a_side_stream_with_an_offset_base(pkg, oracle):
    """A caller-owned buffer whose base is 4-, 8- and 12-byte but not 16-byte aligned under a stride that is a multiple of 16 (the
    route decision looks at the address), and a stride of every residue: all outputs equal, and equal to the restatement's."""
    for stride in ROUTE_STRIDES:
        name = "route:%d" % stride
        rows, end, masks = _case(name)
        for offset in ((0, 4, 8, 12) if stride % 16 == 0 else (0, 8)):
            for mask in masks:
                t, o = _device_find(pkg, rows, end, mask, offset)
                assert _pairs(t, o) == _want(oracle.bsync_find_train_seq, name, mask), (stride, offset, mask)
    for name in ("clamp:4160", "order"):
        rows, end, masks = _case(name)
        t, o = _device_find(pkg, rows, end, ALL, 4)
        assert _pairs(t, o) == _want(oracle.bsync_find_train_seq, name, ALL), name


@pytest.mark.gpu
def test_gpu_scan_device_entry_refuses_bad_arguments(pkg):
    import torch
    dev = torch.device("cuda", 0)
    bits = torch.zeros(4 * 64 + 16, dtype=torch.uint8, device=dev)
    end = torch.full((4,), 40, dtype=torch.int32, device=dev)
    t = torch.zeros(4, dtype=torch.int32, device=dev)
    o = torch.zeros(4, dtype=torch.int32, device=dev)
    dfind = pkg.scan_binding.find_train_seq_batch_device
    ERR_ARG, ERR_ALIGN = -1, -7                               # include/tetra_demod.h
    for args, status in (((bits, 4, 6, end, ALL, t, o), ERR_ALIGN), ((bits.data_ptr() + 1, 4, 64, end, ALL, t, o), ERR_ALIGN),
                         ((None, 4, 64, end, ALL, t, o), ERR_ARG), ((bits, 4, 64, None, ALL, t, o), ERR_ARG),
                         ((bits, 4, 64, end, ALL, None, o), ERR_ARG), ((bits, 4, 64, end, ALL, t, None), ERR_ARG),
                         ((bits, 0, 64, end, ALL, t, o), ERR_ARG)):
        with pytest.raises(pkg.TetraDemodError) as e:
            dfind(*args)
        assert e.value.status == status, (args[1:3], e.value.status)
    torch.cuda.synchronize()
    assert not t.any() and not o.any()


@pytest.mark.gpu
def test_gpu_indicator_equals_the_restatement_across_tile_and_call_edges(pkg, oracle):
    calls = _indicator_schedule()
    ind = pkg.scan_binding.TsIndicator(calls[0][0].shape[0])
    _check_indicator(ind, _indicator_want(oracle))
    ind.close()


@pytest.mark.gpu
def test_gpu_indicator_clamps_its_counts(pkg, oracle):
    calls, want = _clamp_calls(oracle)
    ind = pkg.scan_binding.TsIndicator(4)
    _check_indicator(ind, want, calls)
    ind.close()


@pytest.mark.gpu
def test_gpu_indicator_device_entry_equals_host_entry_and_restatement(pkg, oracle):
    """tetra_ts_indicator_process_device on a side stream, with and without the expire pointer and with d_bits 4 bytes into a torch
    buffer, beside the host entry: the same found / expire as the restatement after every call."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    Cn = 24
    names = list(IND_SEQS)
    hosts = pkg.scan_binding.TsIndicator(Cn)
    devs = [pkg.scan_binding.TsIndicator(Cn) for _ in range(3)]       # (expire pointer, offset): (yes, 0), (NULL, 0), (yes, 4)
    orcs = [oracle.TsIndicatorOracle() for _ in range(Cn)]
    s = torch.cuda.Stream(dev)
    for n in (300, 9000, 44, 17000, 31):
        stride = (n + 11) & ~3
        bits = rng.integers(0, 2, (Cn, stride), dtype=np.uint8)
        bits[:4] = 0
        nb = np.maximum(n - rng.integers(0, 40, Cn), 0).astype(np.int32)
        for c in range(0, Cn, 2):
            q = IND_SEQS[names[(c // 2) % 8]]
            p = int(rng.integers(0, max(1, nb[c] - 20)))
            m = min(len(q), stride - p)
            bits[c, p:p + m] = q[:m]
        want = [o.feed(bits[c, :nb[c]]) for c, o in enumerate(orcs)]
        found, expire = hosts.process(bits, nb)
        assert [(bool(f), int(e)) for f, e in zip(found, expire)] == want, n
        d_nb = torch.from_numpy(nb).to(dev)
        for k, ind in enumerate(devs):
            offset = 4 if k == 2 else 0
            buf = torch.ones(64 + offset + Cn * stride + 64, dtype=torch.uint8, device=dev)
            buf[64 + offset: 64 + offset + Cn * stride] = torch.from_numpy(bits.reshape(-1)).to(dev)
            d_found = torch.full((Cn,), 9, dtype=torch.uint8, device=dev)
            d_expire = torch.full((Cn,), -9, dtype=torch.int32, device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            ind.process_device(buf.data_ptr() + 64 + offset, stride, d_nb, d_found, None if k == 1 else d_expire, s)
            s.synchronize()
            assert [bool(f) for f in d_found.cpu().numpy()] == [f for f, _ in want], (n, k)
            if k == 1:
                assert bool((d_expire == -9).all())
            else:
                assert [int(e) for e in d_expire.cpu().numpy()] == [e for _, e in want], (n, k)
    with pytest.raises(pkg.TetraDemodError) as e:
        devs[0].process_device(buf.data_ptr() + 1, stride, d_nb, d_found, d_expire, s)
    assert e.value.status == -7
    with pytest.raises(pkg.TetraDemodError) as e:
        devs[0].process_device(buf, 6, d_nb, d_found, d_expire, s)
    assert e.value.status == -7
    hosts.close()
    for ind in devs:
        ind.close()
