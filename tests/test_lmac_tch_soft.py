"""TCH/4.8 and TCH/2.4 from soft values (include/ext/tetra_tch_soft.h) without a GPU: the fixture against the reference's own functions
chained as the header defines (tests/tch_soft_definition.py), what the row sets have to hold by the reference alone, the lane code the
kernels run (csrc/tch_soft_core.hpp, compiled for the host by tests/emul/lmac_tch_soft_emul.cpp) bit for bit against the reference on
every set, the header's binding, and the lane code under AddressSanitizer and UBSan."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import tch_definition as td
from tests import tch_soft_definition as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return sd.load_golden()


@pytest.fixture(scope="module")
def emul():
    from tests.emul import lmac_tch_soft_emul_bind
    lmac_tch_soft_emul_bind.build()
    return lmac_tch_soft_emul_bind


@pytest.fixture(scope="module")
def lref(ref):
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not built and the reference is not present")
    return ref.lmac_lib()


def test_fixture_is_what_the_reference_computes(golden, lref):
    """tests/golden/lmac_tch_soft_golden.npz is what tests/golden/make_lmac_tch_soft_golden.py makes: every array, inputs and answers."""
    from tests.golden import make_lmac_tch_soft_golden as G
    again = G.make(lref)
    assert set(again) == set(k for k in golden if not k.endswith("_cols"))
    for k, v in again.items():
        assert v.dtype == golden[k].dtype and np.array_equal(v, golden[k]), k
    assert os.path.getsize(sd.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("kind", sd.CODED)
def test_row_sets_hold_every_case_by_the_reference_alone(golden, kind):
    rows, code, want, be = (golden["%s_%d" % (k, kind)] for k in ("soft", "code", "want", "be"))
    pay = golden["pay_%d" % kind]
    n1, n2 = sd.BLK[kind][2], sd.BLK[kind][1]
    assert rows.shape == (144, 432) and rows.dtype == np.int8 and want.shape == (144, n2) and np.abs(rows.astype(int)).max() == sd.Q == 31
    # clean rows at amplitudes 31, 16, 5, 1 decode to the sent payload, tail zero, nothing differs and everything is compared
    c = sd.set_slice("clean")
    assert [int(np.abs(rows[c][4 * k:4 * k + 4]).max()) for k in range(4)] == [31, 16, 5, 1] and (np.abs(rows[c]).min(axis=1) > 0).all()
    assert np.array_equal(want[c][:, :n1], pay[:16]) and not want[c][:, n1:].any()
    assert np.array_equal(be[c], np.full(16, 432 << 16, np.uint32))
    assert list(code[c][:3]) == [0, 3, 0xffffffff]
    # the all-zero rows decode to zeros and compare nothing; the bound's rows are all +Q, all -Q and the two alternating rows
    z, b = sd.set_slice("zero"), sd.set_slice("bound")
    assert not rows[z].any() and not want[z].any() and not be[z].any()
    alt = np.where(np.arange(432) % 2 == 0, sd.Q, -sd.Q)
    for k, r in enumerate((np.full(432, sd.Q), np.full(432, -sd.Q), alt, -alt)):
        four = slice(b.start + 4 * k, b.start + 4 * k + 4)
        assert (rows[four] == r).all() and list(code[four][:3]) == [0, 3, 0xffffffff] and code[four][3] not in (0, 3, 0xffffffff), k
        assert (be[four] >> 16 == 432).all()
    assert list(code[z][:3]) == [0, 3, 0xffffffff]
    # sparse rows: at most six positions carry a decision
    s = sd.set_slice("sparse")
    assert ((rows[s] != 0).sum(axis=1) <= 6).all() and (be[s] >> 16 <= 6).all() and (be[s] >> 16).max() >= 4
    # the gain set: at least 64 noisy blocks on which the soft definition makes at most half the payload bit errors of the hard one
    g = sd.set_slice("gain")
    assert g.stop - g.start >= 64
    soft_err = int((want[g][:, :n1] != pay[16:16 + 64]).sum())
    hard_err = int((golden["hard_%d" % kind][:, :n1] != pay[16:16 + 64]).sum())
    print("kind %d: payload bit errors soft %d, hard %d" % (kind, soft_err, hard_err))
    assert hard_err >= 50 and 2 * soft_err <= hard_err, (soft_err, hard_err)
    assert len(set(be.tolist())) > 40                    # the counts differ from row to row


@pytest.mark.parametrize("kind", sd.CODED)
def test_hard_rows_of_the_gain_set_are_its_signs(golden, lref, kind):
    """hard_<kind> is tests/tch_definition.decode on the signs, and the soft definition of a clean full-scale row is the hard one's"""
    g = sd.set_slice("gain")
    rows, code = golden["soft_%d" % kind][g], golden["code_%d" % kind][g]
    for b in (0, 31, 63):
        assert np.array_equal(td.decode(lref, kind, sd.hard_rows(rows[b]), code[b]), golden["hard_%d" % kind][b]), b
    c = sd.set_slice("clean").start
    r, cd = golden["soft_%d" % kind][c], golden["code_%d" % kind][c]
    assert np.array_equal(td.decode(lref, kind, sd.hard_rows(r), cd), sd.decode(lref, kind, r, cd))


@pytest.mark.parametrize("counts", (True, False))
@pytest.mark.parametrize("kind", sd.CODED)
def test_lane_code_equals_the_reference_on_every_set_as_rows(golden, emul, kind, counts):
    rows, code = golden["soft_%d" % kind], golden["code_%d" % kind]
    out, be = emul.decode_rows(kind, rows, code, biterr=counts)
    for name, _ in sd.SETS:
        s = sd.set_slice(name)
        assert np.array_equal(out[s], golden["want_%d" % kind][s]), name
        assert be is None if not counts else np.array_equal(be[s], golden["be_%d" % kind][s]), name
    # padded rows (436 bytes apart: no 8-byte alignment), junk in the padding: the same bits
    wide = np.full((len(rows), 436), 0x5a, np.int8)
    wide[:, :432] = rows
    out, be = emul.decode_rows(kind, wide, code, biterr=counts)
    assert np.array_equal(out, golden["want_%d" % kind]) and (be is None or np.array_equal(be, golden["be_%d" % kind]))


@pytest.mark.parametrize("counts", (True, False))
@pytest.mark.parametrize("kind", sd.CODED)
def test_lane_code_equals_the_reference_on_every_set_from_rings(golden, emul, kind, counts):
    """Every row in a ring of its own at the SCH/F burst positions, at every alignment and across the ring's end and the 2^32 wrap of the
    bit number; the smallest ring that holds a burst too.  A frame of another burst type decodes as the all-zero row under its code."""
    rows, code = golden["soft_%d" % kind], golden["code_%d" % kind]
    for ring in (1024, 512):
        out, be = emul.decode_rings(kind, rows, code, biterr=counts, ring=ring)
        assert np.array_equal(out, golden["want_%d" % kind]), ring
        assert be is None if not counts else np.array_equal(be, golden["be_%d" % kind]), ring
    z = sd.set_slice("zero")
    other = np.array([3, 1, 3, 1], np.int32)             # SYNC, NORM_2
    out, be = emul.decode_rings(kind, rows[:4], code[z], biterr=counts, frame_type=other)
    assert np.array_equal(out, golden["want_%d" % kind][z]) and (be is None or not be.any())


def test_header_is_exported_and_bound(pkg):
    """include/ext/tetra_tch_soft.h: the functions it declares are exported by the library and bound with the declared number of
    parameters in lmac_binding.TCH_SOFT_ABI (the ring size as 32 bits, every pointer pointer-wide); the header compiles as C99 and C++11."""
    import re
    import subprocess
    hdr = os.path.join(ROOT, "include", "ext", "tetra_tch_soft.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): [a.strip() for a in " ".join(m.group(2).split()).split(",")] for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    lb = pkg.lmac_binding
    table = lb.TCH_SOFT_ABI
    assert list(decls) == ["tetra_lmac_decode_tch_soft_counted_device", "tetra_lmac_decode_tch_soft_batch", "tetra_lmac_decode_frames_soft_tch_device"]
    assert list(decls) == list(table) == lb.TCH_SOFT_EXPORTS
    L = pkg.load_library()
    lb._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        restype, argtypes = table[name]
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params), name
        for decl, ct in zip(params, argtypes):
            assert C.sizeof(ct) == (C.sizeof(C.c_void_p) if "*" in decl else 4), decl
    assert [len(table[n][1]) for n in decls] == [11, 9, 9]
    # the frame entry takes the parameter list of tetra_lmac_decode_frames_soft_device, the row entries those of their hard siblings
    assert list(table["tetra_lmac_decode_frames_soft_tch_device"][1]) == list(lb.SOFT_ABI["tetra_lmac_decode_frames_soft_device"][1])
    assert list(table["tetra_lmac_decode_tch_soft_counted_device"][1]) == list(lb.TCH_ABI["tetra_lmac_decode_tch_counted_device"][1])
    assert list(table["tetra_lmac_decode_tch_soft_batch"][1]) == list(lb.TCH_ABI["tetra_lmac_decode_tch_batch"][1])
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c++", hdr], check=True)
    # argument checks that need no device: TCH/7.2 and unknown kinds are refused, no rows is a no-op
    for kind in (8, 5, 11, 9 | 0x100):
        assert L.tetra_lmac_decode_tch_soft_counted_device(kind, None, 4, None, 432, None, None, None, 292, None, None) == -1, kind
        assert L.tetra_lmac_decode_tch_soft_batch(kind, None, 4, 432, None, None, 292, None, -1) == -1, kind
    assert L.tetra_lmac_decode_tch_soft_counted_device(9, None, 0, None, 432, None, None, None, 292, None, None) == 0
    assert L.tetra_lmac_decode_tch_soft_counted_device(9, None, 4, None, 432, None, None, None, 292, None, None) == -1


def test_lane_code_is_clean_under_asan_and_ubsan():
    """The same host build as a stand-alone program (tests/san/san_tch_soft.cpp) under AddressSanitizer and UBSan, on exact-size heap
    buffers: both kinds, a ragged workgroup, tight and padded rows, rings that wrap, a frame of another burst type."""
    import subprocess
    from tests.test_sanitizers import ENV, FLAGS, SAN, _stale
    exe = os.path.join(SAN, "san_tch_soft")
    srcs = [os.path.join(SAN, "san_tch_soft.cpp"), os.path.join(ROOT, "tests", "emul", "lmac_tch_soft_emul.cpp")]
    deps = srcs + [os.path.join(ROOT, "tests", "emul", "lmac_lane_io.hpp")] + \
        [os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", f) for f in ("tch_soft_core.hpp", "tch_core.hpp", "soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]
    if _stale(exe, deps):
        subprocess.run(["g++", "-std=c++17", "-Wall"] + FLAGS + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "san_tch_soft: ok" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
