"""Circuit-mode data channels TCH/7.2, TCH/4.8, TCH/2.4 (include/ext/tetra_tch.h) without a GPU: the lane code the kernels run
(csrc/tch_core.hpp, compiled for the host by tests/emul/lmac_tch_emul.cpp) held bit for bit against the reference's own functions
chained as the header defines (tests/tch_definition.py), on the row sets of tests/golden/lmac_tch_golden.npz."""
import os

import numpy as np
import pytest

from tests import tch_definition as td

KINDS = (td.TCH_7_2,) + td.CODED


@pytest.fixture(scope="module")
def golden():
    return td.load_golden()


@pytest.fixture(scope="module")
def tch():
    from tests.emul import lmac_tch_emul_bind
    lmac_tch_emul_bind.build()
    return lmac_tch_emul_bind


@pytest.fixture(scope="module")
def lref(ref):
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not built and the reference is not present")
    return ref.lmac_lib()


def test_golden_file_holds_the_sets_and_is_small(golden):
    assert os.path.getsize(td.GOLDEN) < 512 * 1024
    assert golden["bits"].shape == (200, 432) and set(np.unique(golden["bits"])) == {0, 1}
    b = golden["bytes"]
    assert b.shape == (200, 432)
    for r in b:         # 0, 1, 0xff and 2..254 mixed in every row
        assert (r == 0).any() and (r == 1).any() and (r == 0xff).any() and ((r >= 2) & (r <= 254)).any()
    for kind in td.CODED:
        assert golden["clean_%d" % kind].shape == (64, 432) and golden["noisy_%d" % kind].shape == (64, 432)
        flips = (golden["clean_%d" % kind] != golden["noisy_%d" % kind]).sum(axis=1)
        assert flips.min() == 1 and flips.max() == 40
    for name in ("bits_code", "bytes_code", "code_9", "code_10"):          # scrambling codes 0, 3 and random ones
        c = golden[name]
        assert c[0] == 0 and c[1] == 3 and len(np.unique(c)) == len(c)


def test_golden_file_is_what_the_reference_computes(golden, lref):
    z = td.make_inputs(lref)
    for k, v in z.items():
        assert np.array_equal(v, golden[k]), k
    for k, v in td.expected(lref, z).items():
        assert np.array_equal(v, golden[k]), k


@pytest.mark.parametrize("kind", td.CODED)
def test_clean_blocks_decode_to_the_sent_payload(golden, kind):
    """Known answer: blocks made with the reference's encoder chain, no channel errors."""
    n1 = td.BLK[kind][2]
    want = golden["want_%d_clean" % kind]
    assert np.array_equal(want[:, :n1], golden["pay_%d" % kind])
    assert not want[:, n1:].any()                                           # the tail
    be = golden["be_%d_clean" % kind]
    assert np.array_equal(be, np.full(64, 432 << 16, np.uint32))            # nothing differs, everything compared


@pytest.mark.parametrize("route", (0, 1))
@pytest.mark.parametrize("kind", KINDS)
def test_lane_code_equals_the_reference_on_every_set(golden, tch, kind, route):
    for name, rows, code in td.sets_of(golden, kind):
        out, be, fast = tch.decode_rows(kind, rows, code, route=route, biterr=kind in td.CODED)
        assert np.array_equal(out, golden["want_%d_%s" % (kind, name)]), name
        if kind in td.CODED:
            assert np.array_equal(be, golden["be_%d_%s" % (kind, name)]), name
            # both front-end routes are exercised: plain-bit sets take the packed one unless the byte route is forced
            assert fast == (len(rows) if route == 0 and name != "bytes" else 0), name


@pytest.mark.parametrize("kind", td.CODED)
def test_lane_code_without_counts_and_with_row_padding(golden, tch, kind):
    rows, code = golden["noisy_%d" % kind], golden["code_%d" % kind]
    out, be, _ = tch.decode_rows(kind, rows, code, biterr=False)
    assert be is None and np.array_equal(out, golden["want_%d_noisy" % kind])
    # rows 436 bytes apart are not 8-byte aligned: the byte route, same bits
    wide = np.full((len(rows), 436), 0xa5, np.uint8)
    wide[:, :432] = rows
    out, _, fast = tch.decode_rows(kind, wide, code)
    assert fast == 0 and np.array_equal(out, golden["want_%d_noisy" % kind])


@pytest.mark.parametrize("kind", KINDS)
def test_lane_code_from_packed_frames(golden, tch, kind):
    """The frame front end: NORM_1 frames whose two blocks hold the rows' bits decode like the byte rows; a frame of another burst type
    decodes as the all-zero block."""
    from tests import soft_pipeline as sp
    name = "noisy" if kind in td.CODED else "bits"
    rows = (golden["noisy_%d" % kind] if kind in td.CODED else golden["bits"])[:40]
    code = (golden["code_%d" % kind] if kind in td.CODED else golden["bits_code"])[:40]
    frames = np.zeros((len(rows) + 1, 16), np.uint32)
    pieces = sp.KINDS["schf"][3]
    for b, r in enumerate(rows):
        burst = np.zeros(512, np.uint8)
        at = 0
        for off, ln in pieces:
            burst[off:off + ln] = r[at:at + ln]
            at += ln
        frames[b] = np.packbits(burst).view(">u4").astype(np.uint32)
    frames[-1] = frames[0]
    ftype = np.full(len(rows) + 1, 0, np.int32)        # TETRA_TRAIN_NORM_1
    ftype[-1] = 3                                      # a SYNC burst listed in a TCH job
    scramb = np.concatenate([code, code[:1]])
    n2 = td.BLK[kind][1]
    out, be = tch.decode_frames(kind, frames, ftype, np.arange(len(rows) + 1), scramb, (n2 + 7) & ~7, biterr=kind in td.CODED)
    assert np.array_equal(out[:-1, :n2], golden["want_%d_%s" % (kind, name)][:40])
    zero, zbe, _ = tch.decode_rows(kind, np.zeros((1, 432), np.uint8), code[:1], biterr=kind in td.CODED)
    assert np.array_equal(out[-1, :n2], zero[0])
    if kind in td.CODED:
        assert np.array_equal(be[:-1], golden["be_%d_%s" % (kind, name)][:40]) and be[-1] == zbe[0]


@pytest.mark.parametrize("kind", td.CODED)
def test_step_patterns_are_the_puncturers(tch, lref, kind):
    """The schedule the kernels know (a closed form) against tetra_rcpc_depunct of an all-zero row, and the counts the header states."""
    pat = tch.schedule(kind)
    steps = np.stack([pat >> 4, pat & 0xf], axis=1).reshape(-1)
    assert np.array_equal(steps, td.depunct_patterns(lref, kind))
    count = {p: int((steps == p).sum()) for p in np.unique(steps)}
    if kind == td.TCH_4_8:
        assert count == {0b1100: 146, 0b1000: 140, 0b0000: 6}
    else:
        assert count == {0b1110: 136, 0b1100: 12}


def test_step_pattern_counts_without_the_reference(tch):
    for kind, want in ((td.TCH_4_8, {0b1100: 146, 0b1000: 140, 0b0000: 6}), (td.TCH_2_4, {0b1110: 136, 0b1100: 12})):
        pat = tch.schedule(kind)
        steps = np.stack([pat >> 4, pat & 0xf], axis=1).reshape(-1)
        assert {p: int((steps == p).sum()) for p in np.unique(steps)} == want
        assert sum(bin(p).count("1") for p in steps) == 432


def test_header_is_bound(pkg):
    """The header's symbols are in the binding's call layer; the kinds sit clear of the job flags."""
    import re
    import subprocess
    lb = pkg.lmac_binding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, "include", "ext", "tetra_tch.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): m.group(2).split(",") for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    assert set(decls) == set(lb.TCH_ABI) == {"tetra_lmac_tch_blk_param", "tetra_lmac_decode_tch_counted_device", "tetra_lmac_decode_tch_batch"}
    L = pkg.load_library()
    lb._lib()
    for name, params in decls.items():
        assert len(lb.TCH_ABI[name][1]) == len(params) == len(getattr(L, name).argtypes), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    assert (lb.T_TCH_7_2, lb.T_TCH_4_8, lb.T_TCH_2_4) == (8, 9, 10)
    for k, want in ((8, (432, 432, 432, 0, 0)), (9, (432, 292, 288, 103, 0)), (10, (432, 148, 144, 103, 0))):
        p = lb.tch_blk_param(k)
        assert (p.type345_bits, p.type2_bits, p.type1_bits, p.interleave_a, p.have_crc16) == want
    assert L.tetra_lmac_tch_blk_param(5, None) == -1 and L.tetra_lmac_blk_param(9, None) == -1
    for k in (8, 9, 10):
        assert k & (lb.JOB_RM3014 | lb.JOB_RM3014_SOFT | (0x3ff << 16)) == 0


def test_lane_code_is_clean_under_asan_and_ubsan():
    """The same host build as a stand-alone program (tests/san/san_tch.cpp) under AddressSanitizer and UBSan, on exact-size heap buffers:
    every kind, both routes of the byte rows at a ragged workgroup, tight and padded rows, frames of every burst type."""
    import subprocess
    from tests.test_sanitizers import ENV, FLAGS, SAN, _stale
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(SAN, "san_tch")
    srcs = [os.path.join(SAN, "san_tch.cpp"), os.path.join(root, "tests", "emul", "lmac_tch_emul.cpp")]
    deps = srcs + [os.path.join(root, "tests", "emul", "lmac_lane_io.hpp")] + \
        [os.path.join(root, "sdrpp-tetra-demodulator_amd", "csrc", f) for f in ("tch_core.hpp", "lmac_core.hpp", "demux_core.hpp")]
    if _stale(exe, deps):
        subprocess.run(["g++", "-std=c++17", "-Wall"] + FLAGS + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "san_tch: ok" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
