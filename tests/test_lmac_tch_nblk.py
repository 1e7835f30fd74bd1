"""TCH/4.8 and TCH/2.4 interleaved over N = 1, 4 or 8 blocks (include/ext/tetra_tch_nblk.h) without a GPU: the fixture against the
definition (tests/tch_nblk_definition.py: the clause's transmitter, the header's gather, the reference's functions around it), what the
input sets have to hold by the definition alone, the lane code the kernels run (csrc/tch_nblk_core.hpp, compiled for the host by
tests/emul/lmac_tch_nblk_emul.cpp) bit for bit against the definition on every window, the window helper and the header's binding."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import tch_definition as td
from tests import tch_nblk_definition as nd
from tests import tch_soft_definition as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("hard", "soft")


@pytest.fixture(scope="module")
def golden():
    return nd.load_golden()


@pytest.fixture(scope="module")
def emul():
    from tests.emul import lmac_tch_nblk_emul_bind
    lmac_tch_nblk_emul_bind.build()
    return lmac_tch_nblk_emul_bind


@pytest.fixture(scope="module")
def lref(ref):
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not built and the reference is not present")
    return ref.lmac_lib()


def _case(golden, kind, n, mode):
    tag = dict(nd.cases(kind))[n]
    return (golden[mode + "_" + tag], golden["table_" + tag], golden["index_" + tag], golden["win_%d_%d" % (kind, n)],
            golden["want_%s_%d_%d" % (mode, kind, n)], golden["be_%s_%d_%d" % (mode, kind, n)])


def test_fixture_is_what_the_definition_computes(golden, lref):
    """tests/golden/lmac_tch_nblk_golden.npz is what tests/golden/make_lmac_tch_nblk_golden.py makes: every array, inputs and answers."""
    from tests.golden import make_lmac_tch_nblk_golden as G
    again = G.make(lref)
    assert set(again) == set(k for k in golden if not k.endswith("_cols"))
    for k, v in again.items():
        assert v.dtype == golden[k].dtype and np.array_equal(v, golden[k]), k
    assert os.path.getsize(nd.GOLDEN) < 512 * 1024


def test_transmitter_and_gather_are_each_other_s_inverse(lref):
    """The clause's diagonal interleaver, looped over (m, k), against the receiver's gather: the type-3 block gathered from a transmitted
    stream is the block that went in, for both depths, with a per-row code; and at N = 1 the transmitter is tests/tch_definition.encode."""
    rng = np.random.default_rng(5)
    for kind in nd.CODED:
        n2, n1 = nd.BLK[kind][1], nd.BLK[kind][2]
        pays = rng.integers(0, 2, (5, n1)).astype(np.uint8)
        for n in (1, 4, 8):
            code = 0x1234567 * n
            rows = nd.transmit(lref, kind, pays, n, code)
            assert rows.shape == (5 + n - 1, 432)
            for b in range(5):
                d = np.zeros(n2, np.uint8)
                d[:n1] = pays[b]
                t3 = nd.type3_of(lref, rows, [code] * len(rows), list(range(b, b + n)), len(rows), False)
                assert np.array_equal(t3, nd.encode_type3(lref, kind, d)), (kind, n, b)
            if n == 1:
                assert all(np.array_equal(rows[b], td.encode(lref, kind, pays[b], code)) for b in range(5))
    # the interleaver alone on labelled positions: every position of every block lands exactly once, the head and tail are zero-filled
    for n in (4, 8):
        M = 3
        out = nd.diagonal_interleave(np.ones((M, 432), np.uint8), n)
        assert out.sum() == M * 432 and out[0].sum() == 432 // n and out[-1].sum() == 432 // n and out[n - 1].sum() == min(n, M) * (432 // n)


@pytest.mark.parametrize("n", nd.NS)
@pytest.mark.parametrize("kind", nd.CODED)
def test_sets_hold_every_case_by_the_definition_alone(golden, kind, n):
    n1, n2 = nd.BLK[kind][2], nd.BLK[kind][1]
    win, where = nd.windows_of(n)
    lay = nd.layout(n)
    pay = golden["pay_%d_%d" % (kind, n)]
    assert len(pay) == sum(nd.STREAM_BLOCKS) == 30 and np.array_equal(win, golden["win_%d_%d" % (kind, n)])
    assert 128 < len(win) <= 256 and len(win) % 64 != 0                        # a ragged last workgroup
    assert 90 <= lay["n_rows"] <= 130
    for mode in MODES:
        pool, table, index, _, want, be = _case(golden, kind, n, mode)
        assert pool.shape == (lay["n_rows"], 432) and want.shape == (len(win), n2)
        if mode == "soft":
            assert np.abs(pool.astype(int)).max() == nd.Q
        else:
            assert (pool[:lay["arb"]] <= 1).all() and set(np.unique(pool[lay["arb"]:])) >= {0, 1, 0xff} and len(np.unique(pool[lay["arb"]:])) > 200
        # clean streams return every payload, tail zero, no errors, everything compared
        c = where["clean"]
        assert np.array_equal(want[c][:, :n1], pay) and not want[c][:, n1:].any()
        assert np.array_equal(be[c], np.full(30, 432 << 16, np.uint32))
        # the noisy streams have channel errors
        assert ((be[where["noisy"]] & 0xffff) > 0).all()
        # (a noisy soft value may have rounded to zero: it carries no decision and is not compared)
        assert (be[where["noisy"]] >> 16 == 432).all() if mode == "hard" else (be[where["noisy"]] >> 16 > 400).all()
        # a lost burst at every j: compared drops by 432 / N, and the clean window still returns its payload
        lost = where["lost"]
        assert (be[lost][:n] >> 16 == 432 - 432 // n).all() and lost.stop - lost.start == 2 * n
        assert (be[lost][n:] >> 16 == 432 - 432 // n).all() if mode == "hard" else (be[lost][n:] >> 16 <= 432 - 432 // n).all()
        assert (want[lost][:n, :n1] == pay[2]).all() and not (be[lost][:n] & 0xffff).any()
        # all N lost: a block of erasures, count word 0
        assert be[where["all_lost"]][0] == 0
        # out-of-range entries behave as -1
        o = where["out_of_range"]
        assert (want[o] == want[lost.start + 1]).all() and (be[o] == be[lost.start + 1]).all() and o.stop - o.start == 4
        assert sorted(win[o][:, 1].tolist()) == [nd.INT32_MIN, -7, lay["n_rows"], lay["n_rows"] + 5]
        # a stream with one burst lost returns every payload
        bl = where["burst_lost"]
        assert (win[bl] == -1).sum() == n and np.array_equal(want[bl][:, :n1], pay[-nd.STREAM_BLOCKS[2]:]), (kind, n, mode)
        assert sorted((be[bl] >> 16).tolist())[:n] == [432 - 432 // n] * n
        # the table once more in shuffled order
        assert np.array_equal(want[where["shuffled"]], want[:where["shuffled"].start][where["order"]])
        assert np.array_equal(be[where["shuffled"]], be[:where["shuffled"].start][where["order"]])
        # a window with N different codes, a window naming one row N times
        codes = table[index]
        assert len(set(codes[win[where["odd_any"]][1]].tolist())) == n and len(set(win[where["odd_any"]][0].tolist())) == 1
    # the first workgroup names complete windows of plain-bit rows only
    assert win[:64].min() >= 0 and win[:64].max() < lay["arb"]


@pytest.mark.parametrize("kind", nd.CODED)
def test_depth_1_is_the_single_block_definition(golden, lref, kind):
    """N = 1 with w[0] = b: tests/tch_definition.decode / tests/tch_soft_definition.decode and their count words; a lost row is a block of
    erasures with count word 0."""
    for mode in MODES:
        pool, table, index, win, want, be = _case(golden, kind, 1, mode)
        mod = td if mode == "hard" else sd
        seen = 0
        for b, (r,) in enumerate(win):
            if 0 <= r < len(pool):
                t2 = mod.decode(lref, kind, pool[r], table[index[r]])
                assert np.array_equal(t2, want[b]) and mod.biterr_word(lref, kind, pool[r], table[index[r]], t2) == be[b], (kind, mode, b)
                seen += 1
            else:
                assert be[b] == 0
        assert seen >= 24 and seen < len(win)


@pytest.mark.parametrize("kind", nd.CODED)
def test_the_same_loss_at_depth_1_loses_the_block(lref, kind):
    """One burst of a clean stream lost: at N = 4 and 8 every payload comes back (asserted on the sets above); at N = 1 the block that
    burst carried is gone."""
    n1 = nd.BLK[kind][2]
    rng = np.random.default_rng(77)
    pays = rng.integers(0, 2, (6, n1)).astype(np.uint8)
    rows = nd.transmit(lref, kind, pays, 1, 3)
    soft = (16 * (1 - 2 * rows.astype(np.int32))).astype(np.int8)
    for mode, pool in (("hard", rows), ("soft", soft)):
        for b in range(6):
            t2, word = nd.decode(lref, kind, pool, [3] * 6, [-1 if b == 2 else b], mode == "soft")
            if b == 2:
                assert word == 0 and (t2[:n1] != pays[b]).sum() > n1 // 4, (kind, mode)
            else:
                assert np.array_equal(t2[:n1], pays[b]) and word == 432 << 16


@pytest.mark.parametrize("counts", (True, False))
@pytest.mark.parametrize("n", (1,) + nd.NS)
@pytest.mark.parametrize("kind", nd.CODED)
def test_lane_code_equals_the_definition_on_every_window(golden, emul, kind, n, counts):
    """Rows and count words exact: hard packed route (where a workgroup is entitled to it), hard class route, soft; codes per row and
    through an init index; rows 436 bytes apart with junk between."""
    for mode in MODES:
        pool, table, index, win, want, be = _case(golden, kind, n, mode)
        soft = mode == "soft"
        for route in ((0,) if soft else (0, 1)):
            out, got, fast = emul.decode(kind, n, pool, table[index], win, soft=soft, biterr=counts, route=route)
            assert np.array_equal(out, want), (mode, route)
            assert got is None if not counts else np.array_equal(got, be), (mode, route)
            if not soft:
                assert fast == (64 if route == 0 and n > 1 else 0)
        wide = np.full((len(pool), 436), 0x5a, pool.dtype)
        wide[:, :432] = pool
        out, got, _ = emul.decode(kind, n, wide, table, win, soft=soft, biterr=counts, init_index=index)
        assert np.array_equal(out, want) and (got is None or np.array_equal(got, be)), mode
        # a pool said to be shorter: the rows behind its end are lost
        short = len(pool) - nd.N_ARBITRARY
        out, got, _ = emul.decode(kind, n, pool, table[index], win[:64], soft=soft, biterr=counts, n_rows=short)
        cut = np.where(win[:64] >= short, -1, win[:64])
        out2, got2, _ = emul.decode(kind, n, pool, table[index], cut, soft=soft, biterr=counts)
        assert np.array_equal(out, out2) and (got is None or np.array_equal(got, got2))


def test_class_route_helpers_against_plain_loops(emul):
    """classes_to_bits through the emulation: a workgroup of complete plain windows decodes the same on both routes for random plain pools
    (the packed route is taken), and a single non-plain byte or lost entry anywhere in the workgroup sends all of it the class route."""
    rng = np.random.default_rng(9)
    pool = rng.integers(0, 2, (40, 432)).astype(np.uint8)
    codes = rng.integers(0, 1 << 32, 40, dtype=np.uint64).astype(np.uint32)
    for n in (1, 4, 8):
        win = rng.integers(0, 40, (64, n)).astype(np.int32)
        a = emul.decode(9, n, pool, codes, win, route=0)
        b = emul.decode(9, n, pool, codes, win, route=1)
        assert a[2] == 64 and b[2] == 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] >> 16 == 432).all()
        hurt = win.copy()
        hurt[63, n - 1] = 40
        assert emul.decode(9, n, pool, codes, hurt, route=0)[2] == 0
        dirty = pool.copy()
        dirty[int(win[5, 0]), 103] = 2                       # (type-4 position 103 is the first that diagonal 0 reads, at every depth)
        c = emul.decode(9, n, dirty, codes, win, route=0)
        assert c[2] == 0 and np.array_equal(c[0], emul.decode(9, n, dirty, codes, win, route=1)[0])


def test_window_helper(pkg):
    lb = pkg.lmac_binding
    w = lb.tch_windows([6, 3, 4], 4)
    assert w.dtype == np.int32 and w.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [9, 10, 11, 12]]
    assert lb.tch_windows([6, 3, 4], 4, lost=(2, 12)).tolist() == [[0, 1, -1, 3], [1, -1, 3, 4], [-1, 3, 4, 5], [9, 10, 11, -1]]
    assert lb.tch_windows([3], 1, lost=[1]).tolist() == [[0], [-1], [2]]
    assert lb.tch_windows([], 8).shape == (0, 8) and lb.tch_windows([7, 7], 8).shape == (0, 8)
    assert lb.tch_windows([71], 8).shape == (64, 8)
    for n in nd.NS:              # the sets' sliding streams are what the helper lists
        lay = nd.layout(n)
        assert lb.tch_windows(lay["lengths"], n).tolist() == dict(lay["sets"])["clean"]
    with pytest.raises(ValueError):
        lb.tch_windows([9], 2)


def test_header_is_exported_and_bound(pkg):
    """include/ext/tetra_tch_nblk.h: the functions it declares are exported by the library and bound with the declared number of
    parameters in lmac_binding.TCH_NBLK_ABI (every pointer pointer-wide, everything else 32 bits); the header compiles as C99 and C++11."""
    import re
    import subprocess
    hdr = os.path.join(ROOT, "include", "ext", "tetra_tch_nblk.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): [a.strip() for a in " ".join(m.group(2).split()).split(",")] for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    lb = pkg.lmac_binding
    table = lb.TCH_NBLK_ABI
    assert list(decls) == ["tetra_lmac_decode_tch_nblk_device", "tetra_lmac_decode_tch_nblk_soft_device", "tetra_lmac_decode_tch_nblk_batch",
                           "tetra_lmac_decode_tch_nblk_soft_batch"]
    assert list(decls) == list(table) == lb.TCH_NBLK_EXPORTS
    L = pkg.load_library()
    lb._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        restype, argtypes = table[name]
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params), name
        for decl, ct in zip(params, argtypes):
            assert C.sizeof(ct) == (C.sizeof(C.c_void_p) if "*" in decl else 4), decl
    assert [len(table[n][1]) for n in decls] == [14, 14, 12, 12]
    assert list(table["tetra_lmac_decode_tch_nblk_device"][1]) == list(table["tetra_lmac_decode_tch_nblk_soft_device"][1])
    assert list(table["tetra_lmac_decode_tch_nblk_batch"][1]) == list(table["tetra_lmac_decode_tch_nblk_soft_batch"][1])
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c++", hdr], check=True)
    # argument checks that need no device: TCH/7.2, unknown kinds and depths are refused, no windows is a no-op, windows are needed
    for f in (L.tetra_lmac_decode_tch_nblk_device, L.tetra_lmac_decode_tch_nblk_soft_device):
        for kind in (8, 5, 11, 9 | 0x100):
            assert f(kind, 4, None, 8, 432, None, None, None, 4, None, None, 292, None, None) == -1, kind
        for n in (0, 2, 3, 5, 16, -1):
            assert f(9, n, None, 8, 432, None, None, None, 0, None, None, 292, None, None) == -1, n
        assert f(9, 4, None, 8, 432, None, None, None, 0, None, None, 292, None, None) == 0
        assert f(9, 4, None, 8, 432, None, None, None, 4, None, None, 292, None, None) == -1
        assert f(9, 4, None, -1, 432, None, None, None, 0, None, None, 292, None, None) == -1
    for f in (L.tetra_lmac_decode_tch_nblk_batch, L.tetra_lmac_decode_tch_nblk_soft_batch):
        assert f(8, 4, None, 8, 432, None, None, 4, None, 432, None, -1) == -1
        assert f(9, 2, None, 8, 432, None, None, 0, None, 292, None, -1) == -1
        assert f(10, 8, None, 8, 432, None, None, 0, None, 148, None, -1) == 0
