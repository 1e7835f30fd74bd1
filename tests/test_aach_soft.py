"""The soft AACH decoder (include/ext/tetra_aach_soft.h) without a GPU: the host build of its lane code (tests/emul/aach_soft_emul.cpp: the
staging from the ring, the key with the tie rule, the running best two, the read-out, the row format and the verdict -- the source the
kernels compile) against the numpy definition (tests/aach_soft_definition.py), which stands on the reference encoder's recorded
codewords.  Everything is integer: every comparison is exact.  The GPU tests (tests/test_aach_soft_gpu.py) take their rows from here."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import aach_soft_definition as A
from tests import list_definition as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_NORM_1, TRAIN_NORM_2, TRAIN_SYNC = 0, 1, 3
PIECES = {TRAIN_SYNC: ((252, 30),), TRAIN_NORM_1: ((230, 14), (266, 16)), TRAIN_NORM_2: ((230, 14), (266, 16))}      # tetra_burst.c:343-393
RING = 8192                                      # the chain's minimum ring (soft_core.hpp ring_size)


def emul():
    from tests.emul import aach_soft_emul_bind
    return aach_soft_emul_bind


def padded(values):
    """int [n][30] -> int8 [n][32]"""
    v = np.asarray(values)
    out = np.zeros((len(v), 32), np.int8)
    out[:, :30] = v
    return out


# ---- the rows both suites decode -------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def every_codeword():
    """16384 clean rows at magnitude 1, row i = codeword i"""
    r = padded(1 - 2 * A.code_bits().astype(np.int64))
    r.flags.writeable = False
    return r


@functools.lru_cache(None)
def tie_rows():
    """Codewords with four positions flipped at magnitude 31, the four being half the support of a minimum-weight codeword w: c and
    c ^ w are then both four flips away."""
    bits = A.code_bits()
    light = np.flatnonzero(bits.sum(axis=1) == 8)
    rows = []
    for base, w in ((0, light[0]), (5000, light[1]), (16383, light[-1]), (777, light[len(light) // 2])):
        flip = np.flatnonzero(bits[w])[:4]
        y = 31 * (1 - 2 * bits[base].astype(np.int64))
        y[flip] = -y[flip]
        rows.append(y)
    r = padded(rows)
    r.flags.writeable = False
    return r


@functools.lru_cache(None)
def special_rows():
    """the all-zero row; all values +-31 (codewords at full scale, all +31, all -31, alternating); magnitude-1 values (random signs, sparse)"""
    rng = np.random.default_rng(11)
    bits = A.code_bits()
    rows = [np.zeros(30, np.int64)]
    for info in (0, 1, 8191, 16383, 12345):
        rows.append(31 * (1 - 2 * bits[info].astype(np.int64)))
    alt = np.where(np.arange(30) % 2 == 0, 31, -31)
    rows += [np.full(30, 31), np.full(30, -31), alt, -alt]
    for _ in range(8):
        rows.append(rng.choice((-1, 1), 30))
    for _ in range(8):
        y = np.zeros(30, np.int64)
        y[rng.choice(30, 7, replace=False)] = rng.choice((-1, 1), 7)
        rows.append(y)
    r = padded(rows)
    r.flags.writeable = False
    return r


@functools.lru_cache(None)
def random_rows():
    """2000 rows of the toy channel at each of sigma = 0.45 and 0.65 -> (rows int8 [4000][32], the sent info)"""
    parts = [A.toy_rows(np.random.default_rng(100 + k), 2000, s) for k, s in enumerate((0.45, 0.65))]
    rows, info = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    rows.flags.writeable = False
    return rows, info


@functools.lru_cache(None)
def want(name):
    """the definition's (info, margin, dist) on a named set, computed once"""
    rows = {"every": every_codeword, "tie": tie_rows, "special": special_rows, "random": lambda: random_rows()[0]}[name]()
    out = A.decode(rows)
    for a in out:
        a.flags.writeable = False
    return out


def assert_decodes(rows, name):
    info, margin, dist = want(name)
    words, d, m = emul().decode(rows)
    assert np.array_equal(words, A.codewords()[info]) and np.array_equal(d, dist) and np.array_equal(m, margin), name


# ---- the definition itself means something ------------------------------------------------------------------------------------------
def test_definition_on_the_toy_channel_beats_the_hard_rule():
    """The issue's toy check, restated: at sigma = 0.65 ML returns the sent codeword far more often than the radius-3 rule could (a
    row with more than three hard errors is beyond that rule)."""
    rows, sent = random_rows()
    info, margin, _ = want("random")
    hi = slice(2000, 4000)
    hard_errors = ((rows[hi, :30] < 0) != (A.code_bits()[sent[hi]] != 0)).sum(axis=1)
    ml_right, rm_could = (info[hi] == sent[hi]).sum(), (hard_errors <= 3).sum()
    assert ml_right > rm_could and ml_right >= 1980 and rm_could <= 1900, (ml_right, rm_could)
    assert (margin[hi][info[hi] != sent[hi]] <= 24).all()


# ---- staging ------------------------------------------------------------------------------------------------------------------------
def staging_cases(train):
    """frames of burst type `train` at every alignment, with each piece across the ring's end at every byte, and across 2^32"""
    bn = list(range(8)) + list(range(RING - 300, RING - 220)) + [RING - 1, 0xffffffff, 0xfffffe03, 0xfffffe00 + 231]
    bn = np.array(bn, np.uint64).astype(np.uint32)
    rng = np.random.default_rng(7 + train)
    rings = rng.integers(-31, 32, (len(bn), RING)).astype(np.int8)
    codes = rng.integers(0, 1 << 32, len(bn), dtype=np.uint64).astype(np.uint32)
    codes[:3] = (0, 3, 0xffffffff)
    return rings, bn, codes


def staged_by_numpy(rings, bn, codes, train):
    out = np.zeros((len(bn), 32), np.int8)
    for j in range(len(bn)):
        if train not in PIECES:
            continue                                                       # a foreign burst type: 30 erasures
        idx = np.concatenate([(int(bn[j]) + off + np.arange(ln)) % RING for off, ln in PIECES[train]])
        out[j, :30] = A.descramble(rings[j, idx], D.scramb_seq(codes[j], 30))
    return out


@pytest.mark.parametrize("train", (TRAIN_SYNC, TRAIN_NORM_1, TRAIN_NORM_2, 2, -1))
def test_emulated_staging_and_search_equal_numpy(train):
    rings, bn, codes = staging_cases(train)
    got = emul().stage(rings, bn, np.full(len(bn), train, np.int32), codes)
    exp = staged_by_numpy(rings, bn, codes, train)
    assert np.array_equal(got, exp), train
    assert sorted(set(int(b) % 4 for b in bn)) == [0, 1, 2, 3]
    if train in PIECES:
        assert exp.any() and any(int(b) % RING + off < RING < int(b) % RING + off + ln for b in bn for off, ln in PIECES[train])
    else:
        assert not exp.any()
    rows, ok = emul().rows(got)
    w_rows, w_ok = A.rows(exp)
    assert np.array_equal(rows, w_rows) and np.array_equal(ok, w_ok), train
    if train not in PIECES:
        assert not rows.any() and not ok.any()


# ---- the search on chosen rows ---------------------------------------------------------------------------------------------------------
def test_every_codeword_wins_once():
    info, margin, dist = want("every")
    assert np.array_equal(info, np.arange(16384)) and (margin >= 8).all() and (dist == 0).all()
    assert_decodes(every_codeword(), "every")
    rows, ok = emul().rows(every_codeword())
    assert np.array_equal(rows[:, :30], A.code_bits()) and (rows[:, 30] == 0).all() and np.array_equal(rows[:, 31], margin) and ok.all()


def test_all_zero_row():
    info, margin, dist = (a[0] for a in want("special"))
    assert (info, margin, dist) == (0, 0, 0) and not special_rows()[0].any()
    rows, ok = emul().rows(special_rows()[:1])
    assert not rows.any() and ok[0] == 0


def test_ties_go_to_the_smallest_info():
    info, margin, dist = want("tie")
    y = tie_rows()[:, :30].astype(np.int64)
    corr = y @ (1 - 2 * A.code_bits().astype(np.int64)).T
    for j in range(len(y)):
        tied = np.flatnonzero(corr[j] == corr[j].max())
        assert len(tied) >= 2 and info[j] == tied[0] and margin[j] == 0 and dist[j] == 4, j
    assert (np.abs(y) == 31).all()
    assert_decodes(tie_rows(), "tie")
    assert not emul().rows(tie_rows())[1].any()


def test_extremes():
    info, margin, dist = want("special")
    y = special_rows()[:, :30].astype(np.int64)
    corr = (y * (1 - 2 * A.code_bits()[info].astype(np.int64))).sum(axis=1)
    assert list(info[1:6]) == [0, 1, 8191, 16383, 12345] and (corr[1:6] == 930).all() and (dist[1:6] == 0).all() and (margin[1:6] >= 8 * 31).all()
    assert (np.abs(y[1:10]) == 31).all() and (np.abs(y[10:18]) == 1).all() and (np.abs(y[18:]) <= 1).all() and margin.max() <= A.MAX_MARGIN == emul().max_margin()
    assert_decodes(special_rows(), "special")
    rows, _ = emul().rows(special_rows())
    assert np.array_equal(rows[:, 31], np.minimum(margin, 255)) and (rows[1:6, 31] == 248).all()          # (31 x the minimum distance)


def test_random_rows_equal_numpy():
    assert_decodes(random_rows()[0], "random")
    info, margin, dist = want("random")
    assert (margin == 0).sum() < 40 and margin.max() > 100 and dist.max() >= 4 and (info != random_rows()[1]).any()


def test_verdict_follows_min_margin():
    rows = np.concatenate([random_rows()[0][2000:2600], tie_rows(), special_rows()])
    for mm in (1, 25, 930):
        got_rows, got_ok = emul().rows(rows, mm)
        w_rows, w_ok = A.rows(rows, mm)
        assert np.array_equal(got_rows, w_rows) and np.array_equal(got_ok, w_ok), mm
    ok1, ok25, ok930 = (A.rows(rows, mm)[1] for mm in (1, 25, 930))
    assert ok1.sum() > ok25.sum() >= 500 and ok930.sum() == 0 and (ok1 == 0).sum() >= 5          # (930: see the next test)


def test_margin_930_is_reached_only_by_construction():
    """margin = 930 needs every other codeword at corr <= -930: impossible for a code with more than two words, so min_margin = 930
    refuses everything but is a legal setting; the largest margin of a full-scale codeword is 31 * (minimum distance 8)."""
    _, margin, _ = want("special")
    assert margin[1:6].max() == 31 * 8


# ---- symbols and values -------------------------------------------------------------------------------------------------------------------
def _text(*path):
    return open(os.path.join(ROOT, *path)).read()


def test_symbols_and_values(pkg):
    hdr = _text("include", "ext", "tetra_aach_soft.h")
    assert re.search(r"#define\s+TETRA_LMAC_JOB_RM3014_SOFT\s+0x200\b", hdr)
    assert re.search(r"#define\s+TETRA_LMAC_JOB_AACH_MIN_MARGIN\(m\)\s+\(\(\(m\)\s*&\s*0x3ff\)\s*<<\s*16\)", hdr)
    assert re.search(r"\bTETRA_RX_FLAG_AACH_SOFT\s*=\s*1024\b", _text("include", "tetra_rx.h"))
    assert "tetra_aach_soft.h" in _text("include", "tetra_aach.h") and "tetra_aach_soft.h" in _text("include", "ext", "tetra_soft.h")
    lb, rb = pkg.lmac_binding, pkg.rx_binding
    assert lb.JOB_RM3014_SOFT == 0x200 and lb.job_aach_min_margin(25) == 25 << 16 and lb.job_aach_min_margin(930) == 930 << 16
    assert rb.FLAG_AACH_SOFT == 1024 and callable(lb.rm3014_soft_decode)
    assert callable(rb.RxChain.set_aach_min_margin) and callable(rb.RxChain.fetch_aach_margin)
    assert callable(pkg.wbrx_binding.WidebandRx.set_aach_min_margin) and callable(pkg.wbrx_binding.WidebandRx.fetch_aach_margin)
    bank = _text("sdrpp-tetra-demodulator_amd", "host", "tetra_rx_bank.h")
    assert "setAachMinMargin" in bank and "fetchAachMargin" in bank


def test_extension_header_is_exported_and_bound(pkg):
    """tests/test_abi.py's rule for include/ext/tetra_aach_soft.h: every function it declares is exported by the library and bound with
    the declared number of parameters, every pointer pointer-wide and every other parameter 32 bits; the header compiles as C."""
    hdr = os.path.join(ROOT, "include", "ext", "tetra_aach_soft.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): [a.strip() for a in " ".join(m.group(2).split()).split(",")] for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    table = {**pkg.lmac_binding.AACH_SOFT_ABI, **pkg.rx_binding.AACH_SOFT_ABI}
    assert list(decls) == ["tetra_lmac_rm3014_soft_decode_device", "tetra_rx_set_aach_min_margin", "tetra_rx_fetch_aach_margin"] == list(table)
    L = pkg.load_library()
    pkg.lmac_binding._lib(), pkg.rx_binding._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        restype, argtypes = table[name]
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params), name
        for decl, ct in zip(params, argtypes):
            assert C.sizeof(ct) == (C.sizeof(C.c_void_p) if "*" in decl else 4), decl
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c++", hdr], check=True)
