"""The traffic routing of the receive chain (include/ext/tetra_traffic.h), CPU side: the lane rule of csrc/traffic_core.hpp (host build:
tests/emul/traffic_emul.cpp) against its restatement from the reference's lines (tests/traffic_definition.py) over the whole space of
ACCESS-ASSIGN PDUs, the clamp, the header against the binding, the transmitter of the GPU tests against the reference's own encoder,
and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import chain_host as ch
from tests import tch_definition as td
from tests import traffic_definition as T
from tests.emul import traffic_emul_bind as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ext", "tetra_traffic.h")
ARG, UNSUPPORTED = -1, -2


def _pack_time(tn, fn, mn=1):
    return tn | fn << 8 | mn << 16


def test_lane_rule_equals_the_definition_over_every_access_assign():
    """All 2^14 ACCESS-ASSIGN PDUs x the BBK verdict {0, 1} x fn {1, 17, 18} x the entry's usage {0, 4, 63, the PDU's own field1} x the
    burst types x scrambling code {0, a cell's}: the host build of traffic_core::route gives the definition's kind, case for case.  The
    timeslot (0..5, so that the two values outside 1..4 occur) and the table -- the three kinds and an off entry, rotated -- vary with
    the PDU."""
    pdu = np.arange(1 << 14)
    bits = ((pdu[:, None] >> (13 - np.arange(14))[None, :]) & 1).astype(np.uint8)
    field1 = (pdu >> 6) & 0x3f
    total = routed = 0
    for ok in (0, 1):
        for fn in (1, 17, 18):
            for usage_case in range(4):
                usage = [np.zeros_like(pdu), np.full_like(pdu, 4), np.full_like(pdu, 63), field1][usage_case]
                for ft in (ch.TRAIN_NORM_1, ch.TRAIN_NORM_2, 2, ch.TRAIN_SYNC):
                    for code in (0, 0x0640a517):
                        tn = (pdu + fn + ft) % 6
                        slots = np.zeros((len(pdu), 4, 4), np.uint8)
                        for s in range(4):
                            slots[:, s, 0] = np.array([8, 9, 10, 0])[(pdu // 7 + s) % 4]
                            slots[:, s, 1] = usage
                        slots[:, :, 2:] = 0xa5                      # the padding is not looked at
                        time = _pack_time(tn, fn, 1 + pdu % 60)
                        n = len(pdu)
                        want = T.route_many(np.full(n, ft), np.full(n, code), time, slots, np.full(n, ok), bits)
                        got = E.route(np.full(n, ft), np.full(n, code), time, slots, np.full(n, ok), bits)
                        assert np.array_equal(got, want), (ok, fn, usage_case, ft, code, np.nonzero(got != want)[0][:5])
                        total += n
                        routed += int((want != 0).sum())
    assert total == (1 << 14) * 2 * 3 * 4 * 4 * 2 and 0 < routed < total // 8
    # the vectorised definition is the scalar one (a sample of every case class)
    rng = np.random.default_rng(3)
    for _ in range(3000):
        p = int(rng.integers(0, 1 << 14))
        b = [(p >> (13 - i)) & 1 for i in range(14)]
        slots4 = [(int(rng.choice((0, 8, 9, 10, 7, 11))), int(rng.choice((0, 4, 63, (p >> 6) & 0x3f)))) for _ in range(4)]
        ft, code, ok = int(rng.choice((0, 1, 3))), int(rng.choice((0, 77))), int(rng.integers(0, 2))
        t = _pack_time(int(rng.integers(0, 6)), int(rng.choice((1, 17, 18))))
        s = np.zeros((1, 4, 4), np.uint8)
        s[0, :, 0], s[0, :, 1] = [v[0] for v in slots4], [v[1] for v in slots4]
        want = T.route(ft, code, t, slots4, ok, b)
        assert int(T.route_many([ft], [code], [t], s, [ok], [b])[0]) == want == int(E.route([ft], [code], [t], s, [ok], np.array([b], np.uint8))[0])


def test_usage_gate_is_the_reference_s_is_traffic():
    """Rule (e) by hand on the four headers: header 0 carries no usage marker; markers 1..3 are no traffic (tetra_upper_mac.c:500)."""
    slots4 = [(0, 0), (9, 9), (0, 0), (0, 0)]
    t = _pack_time(2, 5)
    row = lambda hdr, f1: [(hdr >> 1) & 1, hdr & 1] + [(f1 >> (5 - i)) & 1 for i in range(6)] + [0] * 22
    for hdr in range(4):
        for f1 in (0, 3, 9, 10, 63):
            want = 9 if hdr != 0 and f1 == 9 else 0
            assert T.route(0, 5, t, slots4, 1, row(hdr, f1)) == want
            s = np.zeros((1, 4, 4), np.uint8)
            s[0, 1, :2] = (9, 9)
            assert int(E.route([0], [5], [t], s, [1], np.array([row(hdr, f1)], np.uint8))[0]) == want
    assert T.route(0, 5, t, slots4, 0, row(1, 9)) == 0               # an undecodable AACH names nothing
    assert T.route(0, 5, t, [(0, 0), (9, 0), (0, 0), (0, 0)], 0, row(0, 0)) == 9          # no gate: the AACH is not looked at
    assert [T.slot_valid(k, u) for k, u in ((0, 0), (8, 0), (10, 63), (9, 4))] == [True] * 4
    for k in range(0, 256):
        for u in range(0, 256):
            assert E.slot_valid(k, u) == T.slot_valid(k, u), (k, u)
    assert not T.slot_valid(9, 3) and not T.slot_valid(9, 64) and not T.slot_valid(7, 0) and not T.slot_valid(11, 0)


@pytest.mark.parametrize("max_rows", (1, 3, 256, 300))
def test_clamp_keeps_the_first_max_rows_and_counts_the_rest(max_rows):
    """A call's lists as the three kernels leave them (host build): list lengths 0, 1, 255, 256, 257 and max_rows - 1, max_rows,
    max_rows + 1 -- one kind at that length, the other two at other lengths in the same call -- give the first max_rows routed frames in
    (channel, frame) order and routed / kept / dropped to the row."""
    F, Cn = 50, 60
    rng = np.random.default_rng(max_rows)
    for length in sorted({0, 1, 255, 256, 257, max(max_rows - 1, 0), max_rows, max_rows + 1}):
        for kind in T.TCH_KINDS:
            others = [k for k in T.TCH_KINDS if k != kind]
            n = Cn * F
            ft = rng.choice((0, 0, 0, 1, 3, 2), n).astype(np.int32)
            # every channel: timeslots in turn, tn 2 -> kind, tn 4 -> others[0], tn 1 -> others[1] (tn 3 off)
            tn = np.arange(n) % 4 + 1
            time = _pack_time(tn, 1 + (np.arange(n) // 4) % 17)
            table = np.zeros((Cn, 4, 4), np.uint8)
            table[:, 1, 0], table[:, 3, 0], table[:, 0, 0] = kind, others[0], others[1]
            scramb = np.full(n, 9, np.uint32)
            # exactly `length` frames of `kind`: the others that would route lose their scrambling code
            mine = np.nonzero((ft == 0) & (tn == 2))[0]
            assert len(mine) >= length
            scramb[rng.permutation(mine)[length:]] = 0
            any_list = np.nonzero(ft != 2)[0].astype(np.int32)           # (type 2: no burst, not in the ANY list)
            bbk = np.zeros((len(any_list), 32), np.uint8)
            want = {k: [] for k in T.TCH_KINDS}
            for j, r in enumerate(any_list):
                k = T.route(ft[r], scramb[r], time[r], [tuple(int(v) for v in e[:2]) for e in table[r // F]], 1, bbk[j])
                if k:
                    want[k].append(int(r))
            assert len(want[kind]) == length
            lists, counts = E.lists(any_list, F, ft, scramb, time, table, np.ones(len(any_list), np.int32), bbk, max_rows)
            for k in T.TCH_KINDS:
                assert counts[k] == T.clamp(len(want[k]), max_rows), (length, kind, k)
                assert list(lists[k]) == want[k][:max_rows], (length, kind, k)


def _decls():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    return {m.group(2): (m.group(1), [a.strip() for a in " ".join(m.group(3).split()).split(",")])
            for m in re.finditer(r"\b(int|size_t)\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}


def test_traffic_header_is_exported_and_bound(pkg):
    """The five functions include/ext/tetra_traffic.h declares are the binding's RX_TRAFFIC_EXPORTS, exported by the library and bound
    with the declared number of parameters and the declared width of each; no other header's list holds them; the header compiles as
    C99 and C++11; the table entry is four bytes."""
    R = pkg.rx_binding
    decls = _decls()
    assert list(decls) == ["tetra_rx_traffic_enable", "tetra_rx_set_traffic", "tetra_rx_get_traffic", "tetra_rx_fetch_traffic",
                           "tetra_rx_traffic_rows_device"] == R.RX_TRAFFIC_EXPORTS == list(R.TRAFFIC_ABI)
    assert not set(decls) & (set(R.RX_EXPORTS) | set(R.RX_OUT_EXPORTS) | set(R.RX_OUT_EXT_EXPORTS) | set(R.RX_OUT_ROWS_EXPORTS) | set(R.RX_BITERR_EXPORTS))
    L = pkg.load_library()
    R._lib()
    for name, (ret, params) in decls.items():
        fn = getattr(L, name)
        restype, argtypes = R.TRAFFIC_ABI[name]
        assert fn.restype is restype is C.c_int and ret == "int" and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params), name
        for decl, ct in zip(params, argtypes):
            if "*" in decl:
                assert C.sizeof(ct) == C.sizeof(C.c_void_p) and ct is not C.c_int, (name, decl)
            else:
                assert ct is C.c_int and decl.startswith("int "), (name, decl)
    assert [len(decls[n][1]) for n in R.RX_TRAFFIC_EXPORTS] == [2, 5, 4, 10, 9]
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", lang, HDR], check=True)
    prog = '#include "ext/tetra_traffic.h"\nint a[sizeof(tetra_rx_traffic_slot_t) == 4 ? 1 : -1]; int b[TETRA_RX_TRAFFIC_STRIDE(TETRA_LMAC_T_TCH_4_8) == 296 ? 1 : -1];\n'
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=prog.encode(), check=True)
    assert R.TRAFFIC_SLOT_DTYPE.itemsize == 4 and (R.TCH_7_2, R.TCH_4_8, R.TCH_2_4) == T.TCH_KINDS
    assert {k: R.TRAFFIC_TYPE2_BITS[k] for k in T.TCH_KINDS} == {k: td.BLK[k][1] for k in T.TCH_KINDS}
    assert {k: R.TRAFFIC_TYPE1_BITS[k] for k in T.TCH_KINDS} == {k: td.BLK[k][2] for k in T.TCH_KINDS}


def test_traffic_argument_checks_without_a_device(pkg):
    """No handle: TETRA_ERR_ARG from every entry point, before anything touches a device; the table helper of the binding."""
    R = pkg.rx_binding
    L = R._lib()
    n = C.c_int(0)
    assert L.tetra_rx_traffic_enable(None, 5) == ARG
    assert L.tetra_rx_set_traffic(None, 0, 0, None, None) == ARG
    assert L.tetra_rx_get_traffic(None, 0, 0, None) == ARG
    assert L.tetra_rx_fetch_traffic(None, 0, R.TCH_4_8, None, None, 0, 0, None, C.byref(n), None) == ARG
    assert L.tetra_rx_traffic_rows_device(None, 0, R.TCH_4_8, None, None, None, None, None, None) == ARG
    t = R.traffic_table_arg([{2: R.TCH_4_8, 4: (R.TCH_2_4, 17)}, None, {}])
    assert t.shape == (3, 4) and t.dtype == R.TRAFFIC_SLOT_DTYPE and t.tobytes() == bytes([0, 0, 0, 0, 9, 0, 0, 0, 0, 0, 0, 0, 10, 17, 0, 0]) + bytes(32)
    assert R.traffic_table_arg(t) is not None and R.traffic_table_arg(t).tobytes() == t.tobytes()
    with pytest.raises(ValueError):
        R.traffic_table_arg([{5: R.TCH_4_8}])


def test_synth_traffic_option(synth, ref):
    """synth.gen_downlink(traffic=...): without the option the stream is what it is without the parameter, bit for bit; with it only the
    named timeslots' one-channel bursts outside frame 18 change, their blocks are the reference's own encoder chain on the seeded
    payloads (tests/tch_definition.encode), and a gated slot's AACH is the recorded RM(30,14) codeword of header 1, field 1 = usage."""
    a, sa = synth.gen_downlink(T.SLOTS, 31, cell=(7, 8, 9), slot0=T.SLOT0)
    b, sb = synth.gen_downlink(T.SLOTS, 31, cell=(7, 8, 9), slot0=T.SLOT0, traffic=None)
    c, sc = synth.gen_downlink(T.SLOTS, 31, cell=(7, 8, 9), slot0=T.SLOT0, traffic={})
    assert np.array_equal(a, b) and np.array_equal(a, c) and "tch" not in sb and "tch" not in sc
    assert all(np.array_equal(x[1], y[1]) and x[0] == y[0] for k in sa for x, y in zip(sa[k], sb[k]))
    code = synth.tx_scramb_code(7, 8, 9)
    assert code == ref.scramb_get_init(7, 8, 9) if ref.lmac_available() else True
    cw = T.codewords()
    d, sd = synth.gen_downlink(T.SLOTS, 31, cell=(7, 8, 9), slot0=T.SLOT0, traffic={2: (td.TCH_4_8, 9), 4: (td.TCH_7_2, 0), 1: (td.TCH_2_4, 5)}, aach_codewords=cw)
    a, d = a.reshape(-1, 510), d.reshape(-1, 510)
    changed = set(np.nonzero((a != d).any(axis=1))[0].tolist())
    slots = {s: k for s, k, _ in sd["tch"]}
    fn = lambda s: ((s + T.SLOT0) // 4) % 18 + 1
    tn = lambda s: (s + T.SLOT0) % 4 + 1
    assert changed == set(slots) == {s for s in range(T.SLOTS) if tn(s) in (2, 4) and fn(s) != 18}
    assert any(fn(s) == 18 for s in range(T.SLOTS)) and {slots[s] for s in slots if tn(s) == 2} == {td.TCH_4_8}
    assert sorted(s for s, _ in sd["schf"]) == sorted(s for s in range(T.SLOTS) if tn(s) in (2, 4) and fn(s) == 18)
    # seeded apart from the rest: the same payloads whatever else the stream holds
    _, se = synth.gen_downlink(T.SLOTS, 31, cell=(1, 2, 3), slot0=T.SLOT0, traffic={2: (td.TCH_4_8, 0), 4: (td.TCH_7_2, 0)})
    assert all(np.array_equal(x[2], y[2]) for x, y in zip(sd["tch"], se["tch"]))
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not available: the encoder is not held against the reference here")
    L = ref.lmac_lib()
    seq = np.zeros(30, np.uint8)
    L.tetra_scramb_bits(code, seq.ctypes.data_as(C.c_void_p), 30)
    for s, kind, pay in sd["tch"]:
        burst = d[s]
        if kind == td.TCH_7_2:
            want = pay.copy()
            L.tetra_scramb_bits(code, want.ctypes.data_as(C.c_void_p), 432)
        else:
            want = td.encode(L, kind, pay, code)
        assert np.array_equal(ch.cut(burst, 0, T.SCHF_PIECES), want), (s, kind)
        assert np.array_equal(burst[244:266], synth.TRAIN_NORM_1)
        aach = ch.cut(burst, 0, ch.BLOCK[(ch.TRAIN_NORM_1, ch.KIND_BBK)].pieces) ^ seq
        if tn(s) == 2:
            word = int(cw[1 << 12 | 9 << 6])
            assert list(aach) == [(word >> (29 - i)) & 1 for i in range(30)] and T.access_assign(aach) == 9
        else:
            assert np.array_equal(aach, dict(sa["bbk"])[s])
    for kind in T.TCH_KINDS:                       # the encoder itself, on more rows and codes
        rng = np.random.default_rng(kind)
        pay = rng.integers(0, 2, (24, td.BLK[kind][2])).astype(np.uint8)
        codes = td.codes(rng, 24)
        got = synth.tx_encode_tch(kind, pay, codes)
        for j in range(24):
            if kind == td.TCH_7_2:
                want = pay[j].copy()
                L.tetra_scramb_bits(int(codes[j]), want.ctypes.data_as(C.c_void_p), 432)
            else:
                want = td.encode(L, kind, pay[j], codes[j])
            assert np.array_equal(got[j], want), (kind, j)


def test_the_gpu_tests_stream_is_decodable_by_the_reference_alone(synth, oracle, ref):
    """The mixed table's stream at the synth's default level (seed chosen on the CPU, from this pipeline alone: of the seeds 7400, 7410,
    .. 7790, 19 leave no miss; 7410 routes the most rows): the reference-only pipeline returns every routed block's payload as it was
    sent, under every AACH rule and from hard and soft values, and the table exercises all three kinds, gated and ungated entries."""
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not available")
    from tests import soft_pipeline as SP
    cells, tx, iq = T.downlink(synth, T.MIXED)
    streams = SP.oracle_streams(oracle, iq)
    for flags in (0, T.SOFT, T.AACH_RM3014, T.SOFT | T.AACH_SOFT):
        rows = T.stream_rows(ref, oracle, iq, T.MIXED, flags, streams)
        assert {k: len(v) for k, v in rows.items()} == {8: 14, 9: 14, 10: 15}, flags
        T.assert_payloads(rows, tx)
