"""CRC-aided list decoding of CRC-failed blocks (include/ext/tetra_list.h) against an independent numpy statement of its definition
(tests/list_definition.py: a plain Viterbi decoder that stores every decision and every difference).  The damaged rows come from the
REFERENCE's encoder with fixed seeds (tests/golden/make_list_golden.py -> tests/golden/list_golden.npz, which also holds the reference's
own decoding of each row); where oracle/_ref is built the fixture is made again and has to come out the same.

One condition the feature's request lists for the rows cannot hold under the definition it fixes, "a winning flip in step 0 or 1": the
decision at step t only chooses bit 0 of the state after step t - 1, which is the input bit of step t - 4, so candidates of steps 0..3
change no decoded bit and always fail the CRC again (test_flips_in_the_first_four_steps_change_no_bit shows it on every failed row).  The
rows hold the earliest flips that can win instead, steps 4 and 5, which change decoded bits 0 and 1."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import list_definition as D
from tests.golden import make_list_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS = (1, 4, 8)
N_ERASED0 = G.N_CLEAN + G.N_NOISY                     # first row with erasures
SOFT_T = {"sb1": 0, "sb2": 1, "ndb1": 2, "ndb2": 2, "schf": 5}
FRAME_JOBS = ((5, 0, 0), (1, 2, 3), (2, 1, 1), (2, 2, 1), (0, 1, 3))          # (tpsap, blk_num, carrying burst type)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


def for_T(d, T):
    """A definition result computed with eight candidates, cut down to T: the order does not depend on T."""
    rank = np.where((d["rank"] > 0) & (d["rank"] <= T), d["rank"], np.where(d["rank"] == 0, 0, -1)).astype(np.int32)
    out = np.where((rank > 0)[:, None], d["out"], d["ml"])
    return out, (rank >= 0).astype(np.int32), rank


@pytest.fixture(scope="module")
def golden():
    g = np.load(G.PATH)
    return _freeze({k: g[k] for k in g.files})


@pytest.fixture(scope="module")
def hard(golden):
    """Per coded kind: the golden rows, the reference's decoding and the definition's result with eight candidates.  Read-only."""
    pool = {}
    for t in G.CODED:
        rows, si = golden["hard%d_rows" % t], golden["hard%d_si" % t]
        d = D.list_decode(t, D.hard_values(t, rows, si), 8, D.START_HARD)
        pool[t] = _freeze(dict(d, rows=rows, si=si, want=golden["hard%d_want" % t], want_ok=golden["hard%d_ok" % t]))
    return pool


@pytest.fixture(scope="module")
def soft(golden):
    pool = {}
    for kind, t in SOFT_T.items():
        sv, si = golden["soft_%s_soft" % kind], golden["soft_%s_si" % kind]
        d = D.list_decode(t, D.soft_values(t, sv, si), 8, D.START_SOFT)
        pool[kind] = _freeze(dict(d, t=t, soft=sv, si=si, want=golden["soft_%s_want" % kind], want_ok=golden["soft_%s_ok" % kind]))
    return pool


def unpack_frames(golden):
    frames = np.unpackbits(golden["frames_bits"], axis=1)
    words = np.packbits(frames, axis=1).view(">u4").astype(np.uint32)               # 16 words per frame, first bit most significant
    return frames, words, golden["frames_types"], golden["frames_codes"]


def frame_rows(golden, oracle, tpsap, blk, listed):
    """The demultiplexed type-5 rows of the listed frames for one kind (a frame of another burst type: the all-zero row)."""
    frames, _, types, codes = unpack_frames(golden)
    n345 = D.BLK[tpsap][0]
    rows = np.zeros((len(listed), n345), np.uint8)
    for j, r in enumerate(listed):
        row = oracle.bsync_demux(frames[r], int(types[r]), tpsap, blk) if types[r] >= 0 else np.zeros(0, np.uint8)
        rows[j, :row.size] = row
    return rows, codes[listed]


def listed_frames(types, train):
    carrying = [r for r in range(len(types)) if types[r] == train]
    return np.array(carrying + [r for r in range(len(types)) if types[r] != train][:5], np.int32)


# ---- the fixture and the definition ---------------------------------------------------------------------------------------------------------
def test_the_golden_rows_are_the_reference_encoders_and_the_ml_path_is_the_reference_decoders(golden, hard, soft):
    """The definition's ML path and verdict equal the reference's lmac_decode (soft values: conv_cch_decode) on every row; where
    oracle/_ref is built the whole fixture is made again from the reference's encoder and decoder and equals the committed file."""
    for t in G.CODED:
        assert np.array_equal(hard[t]["ml"], hard[t]["want"]) and np.array_equal(hard[t]["ml_ok"], hard[t]["want_ok"]), t
    for kind, s in soft.items():
        assert np.array_equal(s["ml"], s["want"]) and np.array_equal(s["ml_ok"], s["want_ok"]), kind
    from oracle import ref_binding
    if ref_binding.available() and ref_binding.lmac_available():
        again = G.make(ref_binding)
        assert set(again) == set(golden)
        for k in again:
            assert np.array_equal(again[k], golden[k]), k


def test_the_chosen_rows_hold_every_case_of_the_definition(hard, soft):
    """By the definition alone the rows contain: winners at rank 1 and at rank >= 3, rows no candidate rescues, a tie in Delta among the
    first four candidates of a failed row, winning flips in an even and in an odd step, in the earliest steps that can win (4 or 5), in
    flush steps, failed rows with 0xff erasures (rescued and not), and rows rescued only by T = 8."""
    for t in G.CODED:
        h = hard[t]
        n2 = D.BLK[t][1]
        rank, win, failed = h["rank"], h["win_step"], h["ml_ok"] == 0
        assert (rank == 1).sum() >= 5 and (rank >= 3).sum() >= 3 and (rank == -1).sum() >= 10 and (rank == 0).sum() >= G.N_CLEAN, t
        assert (rank > 4).any(), t
        first4 = np.take_along_axis(h["delta"], h["order"][:, :4], 1)
        assert (failed & (np.diff(first4, axis=1) == 0).any(1)).sum() >= 10, t
        assert ((win >= 0) & (win % 2 == 0)).any() and ((win >= 0) & (win % 2 == 1)).any(), t
        assert (win >= n2).any(), t                                   # a flush step, in every kind
        erased = slice(N_ERASED0, N_ERASED0 + G.N_ERASED)
        assert (rank[erased] > 0).any() and (rank[erased] == -1).any(), t
        assert h["ml_ok"][:G.N_CLEAN].all()
    wins = np.concatenate([hard[t]["win_step"] for t in G.CODED])
    last = np.concatenate([hard[t]["win_step"] - D.BLK[t][1] for t in G.CODED])
    assert (wins == 4).any() and (wins == 5).any()
    assert (last >= 0).any() and last.max() >= 2                     # flush steps (the last block step would be -1)
    for kind, s in soft.items():
        assert (s["rank"] == 1).sum() >= 5 and (s["rank"] >= 2).sum() >= 3 and (s["rank"] == -1).sum() >= 3 and (s["rank"] == 0).sum() >= 10, kind


def test_flips_in_the_first_four_steps_change_no_bit(hard):
    """Why no flip in steps 0..3 can win: the definition's own candidate traceback with such a flip returns the ML bits on every row."""
    t = 0
    h = hard[t]
    v3 = D.hard_values(t, h["rows"], h["si"])
    n2 = D.BLK[t][1]
    for step in range(4):
        d = D.list_decode(t, v3, 8, D.START_HARD, forced_first=step)
        assert np.array_equal(d["first_bits"][:, :n2], h["ml"]), step
    d = D.list_decode(t, v3, 8, D.START_HARD, forced_first=4)
    assert (d["first_bits"][:, 0] != h["ml"][:, 0]).all()


def test_the_rescue_never_loses_a_block(hard, soft):
    for pool in (hard, soft):
        for h in pool.values():
            for T in TS:
                _, ok, rank = for_T(h, T)
                assert (ok >= h["ml_ok"]).all() and ((rank > 0) == (ok > h["ml_ok"])).all()


# ---- the lane code, through the host emulation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", G.CODED)
def test_lane_code_equals_the_definition_on_byte_rows(hard, t):
    """list_core.hpp built for the host behind k_lmac_decode's front ends and the rescue launch's: the packed route where a workgroup's
    rows are plain bits, the byte route elsewhere (the workgroup with the erasures) and forced for every row, T = 1, 4, 8: rows,
    verdicts and ranks are the definition's on every row; on plain rows a rescue that stages packed bits gives the same again."""
    from tests.emul import lmac_list_emul_bind as E
    h = hard[t]
    n345 = D.BLK[t][0]
    rows = np.zeros((len(h["rows"]), 440), np.uint8)
    rows[:, :n345] = h["rows"]
    for T in TS:
        want, want_ok, want_rank = for_T(h, T)
        for route in (0, 1):
            out, ok, rank, _ = E.decode_rows(t, rows, h["si"], T, route)
            assert np.array_equal(rank, want_rank) and np.array_equal(ok, want_ok) and np.array_equal(out, want), (t, T, route)
        plain = slice(0, 64)
        out, ok, rank, _ = E.decode_rows(t, rows[plain], h["si"][plain], T, 0, bits_rescue=True)
        assert np.array_equal(rank, want_rank[plain]) and np.array_equal(out, want[plain]), (t, T)
    assert (want_rank[:64] > 0).any()


def test_lane_code_equals_the_definition_on_packed_frames(golden, oracle):
    """... behind k_lmac_frames' front end: frames of every burst type, a few listed under a kind they do not carry."""
    from tests.emul import lmac_list_emul_bind as E
    _, words, types, codes = unpack_frames(golden)
    rescued = 0
    for tpsap, blk, train in FRAME_JOBS:
        listed = listed_frames(types, train)
        rows, rc = frame_rows(golden, oracle, tpsap, blk, listed)
        d = D.list_decode(tpsap, D.hard_values(tpsap, rows, rc), 8, D.START_HARD)
        for T in TS:
            want, want_ok, want_rank = for_T(d, T)
            out, ok, rank, _ = E.decode_frames(tpsap, blk, words, types, listed, None if tpsap == 0 else codes, D.BLK[tpsap][1], T)
            assert np.array_equal(rank, want_rank) and np.array_equal(ok, want_ok) and np.array_equal(out, want), (tpsap, blk, T)
        rescued += int((want_rank > 0).sum())
        assert (want_rank == -1).any() and (want_rank == 0).any()
    assert rescued >= 10


@pytest.mark.parametrize("kind", sorted(SOFT_T))
def test_lane_code_equals_the_definition_on_soft_values(soft, kind):
    """... behind k_lmac_frames_soft's front end: the rows laid into rings at bit numbers that make them wrap."""
    from tests.emul import lmac_list_emul_bind as E
    s = soft[kind]
    for T in TS:
        want, want_ok, want_rank = for_T(s, T)
        out, ok, rank, _ = E.decode_soft_rows(kind, s["soft"], None if s["t"] == 0 else s["si"], T)
        assert np.array_equal(rank, want_rank) and np.array_equal(ok, want_ok) and np.array_equal(out, want), (kind, T)


def test_rescued_rows_count_bit_errors_on_the_rescued_codeword(hard):
    """With counts, a row's errors | compared << 16 is the distance of the received row to the codeword of the bits the row ends up
    with -- the rescued ones where a candidate won -- as the definition of tetra_biterr.h gives it (restated in numpy)."""
    from tests.emul import lmac_list_emul_bind as E
    for t in (0, 5):
        h = hard[t]
        out, ok, rank, be = E.decode_rows(t, h["rows"], h["si"], 8, 1)
        assert (rank > 0).sum() >= 20 and np.array_equal(out, h["out"])
        for b in range(len(out)):
            assert (int(be[b]) & 0xffff, int(be[b]) >> 16) == D.count_errors(t, h["rows"][b], h["si"][b], out[b]), (t, b)
        changed = [b for b in np.flatnonzero(rank > 0) if D.count_errors(t, h["rows"][b], h["si"][b], h["ml"][b]) != D.count_errors(t, h["rows"][b], h["si"][b], out[b])]
        assert len(changed) >= 3                 # a count left at the ML row's value would be noticed (many winners tie with the ML path: Delta = 0)


def test_extension_header_is_exported_and_bound(pkg):
    """tests/test_abi.py's rule for include/ext/tetra_list.h: every function it declares is exported by the library and has an entry with as
    many parameters in a binding module's LIST_ABI table; the header compiles as C."""
    import re
    import subprocess
    hdr = os.path.join(ROOT, "include", "ext", "tetra_list.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): [a for a in " ".join(m.group(2).split()).split(",")] for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    tables = {**pkg.lmac_binding.LIST_ABI, **pkg.rx_binding.LIST_ABI}
    assert len(decls) == 6 and set(decls) == set(tables)
    L = pkg.load_library()
    pkg.lmac_binding._lib(), pkg.rx_binding._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        assert len(tables[name][1]) == len(params) == len(fn.argtypes), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    text = open(hdr).read()
    assert "TETRA_LIST_MAX_CANDIDATES 8" in text and "TETRA_LIST_DEFAULT_CANDIDATES 4" in text
    assert (pkg.lmac_binding.LIST_MAX_CANDIDATES, pkg.lmac_binding.LIST_DEFAULT_CANDIDATES) == (8, 4)
    assert "TETRA_RX_FLAG_LIST = 512" in open(os.path.join(ROOT, "include", "tetra_rx.h")).read() and pkg.rx_binding.FLAG_LIST == 512


def test_lane_code_is_clean_under_asan_and_ubsan():
    """The same host build as a stand-alone program (tests/san/san_list.cpp) under AddressSanitizer and UBSan, on exact-size heap
    buffers: both routes of the byte rows at a ragged workgroup, frames of every burst type, soft values from rings that wrap."""
    import subprocess
    from tests.test_sanitizers import ENV, FLAGS, SAN, _stale
    exe = os.path.join(SAN, "san_list")
    srcs = [os.path.join(SAN, "san_list.cpp"), os.path.join(ROOT, "tests", "emul", "lmac_list_emul.cpp")]
    deps = srcs + [os.path.join(ROOT, "tests", "emul", "lmac_lane_io.hpp")] + \
        [os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", f) for f in ("list_core.hpp", "lmac_core.hpp", "soft_core.hpp", "demux_core.hpp")]
    if _stale(exe, deps):
        subprocess.run(["g++", "-std=c++17", "-Wall"] + FLAGS + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "san_list: ok" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5a5a5a5a
ERR_ARG, ERR_ALIGN = -1, -7                              # include/tetra_demod.h


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _u32(torch, a, dev):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).to(dev)


def _pick(h, n, pattern):
    """n row indices of a pool: no failed row, only failed rows, or exactly one failed row per 64 (at a different lane each)."""
    good, bad = np.flatnonzero(h["ml_ok"] == 1), np.flatnonzero(h["ml_ok"] == 0)
    if pattern == "none":
        return np.resize(good, n)
    if pattern == "all":
        return np.resize(bad, n)
    if pattern == "one_per_wave":
        idx = np.resize(good, n)
        for w in range((n + 63) // 64):
            at = min(64 * w + (17 * w + 5) % 64, n - 1)
            idx[at] = bad[(3 * w) % len(bad)]
        return idx
    return np.resize(np.arange(len(h["ml_ok"])), n)                # "mixed": the pool in order


@pytest.mark.gpu
@pytest.mark.parametrize("t", (0, 4, 2, 5))
def test_gpu_byte_rows_equal_the_emulation(pkg, hard, t):
    """tetra_lmac_decode_counted_list_device on SB1, SCH/HU, NDB and SCH/F rows: 1, 63, 64, 65 and 130 rows (ragged 64-row workgroups) with
    no failed row, only failed rows, exactly one per wave and the pool in order (which crosses into the rows with erasures), both routes
    of the front end, T = 4 (T = 1 and 8 on the mixed rows): rows, verdicts and ranks equal the host emulation's -- and so the
    definition's -- on every row; padding bytes of the output rows are not touched."""
    from tests.emul import lmac_list_emul_bind as E
    torch, dev = _dev()
    lb = pkg.lmac_binding
    h = hard[t]
    n345, n2 = D.BLK[t][:2]
    ost = lb.out_stride_for(t) + 8
    stride = n345 + (-n345) % 8
    rescued = 0
    for n in (1, 63, 64, 65, 130):
        for pattern in ("none", "all", "one_per_wave", "mixed"):
            idx = _pick(h, n, pattern)
            rows = np.zeros((n, stride), np.uint8)
            rows[:, :n345] = h["rows"][idx]
            si = h["si"][idx]
            d_rows, d_si = torch.from_numpy(rows).to(dev), (None if t == 0 else _u32(torch, si, dev))
            for T in ((1, 4, 8) if pattern == "mixed" and n == 130 else (4,)):
                for forced in (False, True):
                    want, want_ok, want_rank, _ = E.decode_rows(t, rows, si, T, int(forced))
                    d_want, d_ok, d_rk = for_T({k: h[k][idx] for k in ("rank", "out", "ml")}, T)
                    assert np.array_equal(want, d_want) and np.array_equal(want_rank, d_rk)
                    t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
                    ok = torch.full((n,), -3, dtype=torch.int32, device=dev)
                    rk = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
                    lb.force_byte_route(forced)
                    try:
                        lb.decode_counted_list_device(t, d_rows, n, None, stride, d_si, None, t2, ost, ok, T, rk)
                        torch.cuda.synchronize()
                    finally:
                        lb.force_byte_route(False)
                    got = t2.cpu().numpy()
                    assert np.array_equal(rk.cpu().numpy(), want_rank), (t, n, pattern, T, forced)
                    assert np.array_equal(ok.cpu().numpy(), want_ok) and np.array_equal(got[:, :n2], want), (t, n, pattern, T, forced)
                    assert (got[:, n2 + (-n2) % 4:] == 7).all()
                    rescued += int((want_rank > 0).sum())
    assert rescued > 50
    # the counted form: a device-side count below the capacity; rows past it keep their sentinels
    n, have = 130, 70
    idx = _pick(h, n, "all")
    rows, si = np.ascontiguousarray(h["rows"][idx]), h["si"][idx]
    t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
    ok = torch.full((n,), -3, dtype=torch.int32, device=dev)
    rk = torch.full((n,), SENTINEL, dtype=torch.int32, device=dev)
    lb.decode_counted_list_device(t, torch.from_numpy(rows).to(dev), n, torch.tensor([have], dtype=torch.int32, device=dev), n345,
                                  None if t == 0 else _u32(torch, si, dev), None, t2, ost, ok, 8, rk)
    torch.cuda.synchronize()
    want, want_ok, want_rank, _ = E.decode_rows(t, rows[:have], si[:have], 8, 0)
    assert (rk[have:] == SENTINEL).all() and (ok[have:] == -3).all() and (t2[have:] == 7).all()
    assert np.array_equal(rk.cpu().numpy()[:have], want_rank) and np.array_equal(ok.cpu().numpy()[:have], want_ok)
    assert np.array_equal(t2.cpu().numpy()[:have, :n2], want) and (want_rank > 0).any() and (want_rank == -1).any()


@pytest.mark.gpu
def test_gpu_byte_rows_host_entry_null_rank_and_argument_errors(pkg, hard):
    """tetra_lmac_decode_batch_list (host pointers) rescues the same rows; a NULL rank array is the existing entry point, byte for byte; a
    rank array for the AACH and T outside 1..8 are TETRA_ERR_ARG, a misaligned rank array TETRA_ERR_ALIGN."""
    from tests.emul import lmac_list_emul_bind as E
    torch, dev = _dev()
    lb = pkg.lmac_binding
    h = hard[5]
    t2, ok, rank = lb.decode_batch_list(5, h["rows"], h["si"], 4)
    want, want_ok, want_rank = for_T(h, 4)
    assert np.array_equal(rank, want_rank) and np.array_equal(ok, want_ok) and np.array_equal(t2[:, :288], want)
    plain, plain_ok = lb.decode_batch(5, h["rows"], h["si"])
    assert np.array_equal(plain[:, :288], h["ml"]) and np.array_equal(plain_ok, h["ml_ok"])
    L = pkg.binding.load_library()
    rows = torch.from_numpy(np.array(h["rows"][:70])).to(dev)
    si = _u32(torch, h["si"][:70], dev)
    out = torch.zeros((70, 288), dtype=torch.uint8, device=dev)
    okd = torch.zeros(70, dtype=torch.int32, device=dev)
    rk = torch.zeros(72, dtype=torch.int32, device=dev)
    f = L.tetra_lmac_decode_counted_list_device
    args = (rows.data_ptr(), 70, None, 432, si.data_ptr(), None, out.data_ptr(), 288, okd.data_ptr())
    assert f(3, *args, 4, rk.data_ptr(), None) == ERR_ARG
    assert f(5, *args, 0, rk.data_ptr(), None) == ERR_ARG and f(5, *args, 9, rk.data_ptr(), None) == ERR_ARG
    assert f(5, *args, 4, rk.data_ptr() + 2, None) == ERR_ALIGN
    assert f(5, *args, 0, None, None) == 0                        # no rank array: T is not looked at, the rows are the decoder's
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), h["ml"][:70]) and np.array_equal(okd.cpu().numpy(), h["ml_ok"][:70])
    assert f(5, *args, 8, rk.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(rk.cpu().numpy()[:70], for_T(h, 8)[2][:70])
    fb = L.tetra_lmac_decode_batch_list
    r4 = np.zeros(4, np.int32)
    z = np.zeros((4, 432), np.uint8)
    o, k4, s4 = np.zeros((4, 288), np.uint8), np.zeros(4, np.int32), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert fb(5, p(z), 4, 432, p(s4), p(o), 288, p(k4), 9, p(r4), 0) == ERR_ARG
    assert fb(3, p(z), 4, 432, p(s4), p(o), 288, p(k4), 4, p(r4), 0) == ERR_ARG


@pytest.mark.gpu
def test_gpu_frames_equal_the_byte_row_route(pkg, golden, oracle):
    """tetra_lmac_decode_frames_list_device: one launch with SCH/F, SB2, NDB 1, NDB 2 and BBK jobs over 104 frames of all burst types, NDB 2
    with a NULL rank entry.  Rescued jobs: rows, verdicts, ranks and the labels' crc_ok equal the emulation's and the byte-row entry
    point's on the demultiplexed rows, row for row; the job without ranks and the AACH job are what tetra_lmac_decode_frames_device
    writes; a rank entry for the AACH is TETRA_ERR_ARG."""
    from tests.emul import lmac_list_emul_bind as E
    torch, dev = _dev()
    lb = pkg.lmac_binding
    _, words, types, codes = unpack_frames(golden)
    nf = len(types)
    d_frames = _u32(torch, words, dev)
    d_types = torch.from_numpy(types).to(dev)
    d_codes = _u32(torch, codes, dev)
    d_bitnum = _u32(torch, np.arange(nf) * 510 + 7, dev)
    d_time = _u32(torch, np.arange(nf) + 100, dev)
    kinds = ((5, 0, 0), (1, 2, 3), (2, 1, 1), (2, 2, 1), (3, 0, None))
    T = 4

    def jobs_for(with_rank):
        jobs = []
        for tpsap, blk, train in kinds:
            listed = np.arange(nf, dtype=np.int32) if train is None else listed_frames(types, train)
            n, ost = len(listed), 32 if tpsap == 3 else D.BLK[tpsap][1]
            jobs.append(dict(type=tpsap, blk_num=blk, row_frame=torch.from_numpy(listed).to(dev), n_rows=None, max_rows=n, out_stride=ost, frame_scramb=d_codes,
                             type2=torch.full((n, ost), 7, dtype=torch.uint8, device=dev), crc_ok=torch.full((n,), -3, dtype=torch.int32, device=dev),
                             labels=torch.zeros((n, 6), dtype=torch.int32, device=dev),
                             rank=torch.full((n,), SENTINEL, dtype=torch.int32, device=dev) if with_rank and tpsap != 3 and (tpsap, blk) != (2, 2) else None,
                             listed=listed))
        return jobs

    jobs, plain = jobs_for(True), jobs_for(False)
    lb.decode_frames_list_device(d_frames, d_types, jobs, T, frames_per_channel=nf, d_frame_bitnum=d_bitnum, d_time_rx=d_time, d_time=d_time)
    lb.decode_frames_device(d_frames, d_types, plain, frames_per_channel=nf, d_frame_bitnum=d_bitnum, d_time_rx=d_time, d_time=d_time)
    torch.cuda.synchronize()
    rescued = 0
    for j, q, (tpsap, blk, train) in zip(jobs, plain, kinds):
        rows_g, ok_g, lab_g = j["type2"].cpu().numpy(), j["crc_ok"].cpu().numpy(), j["labels"].cpu().numpy()
        lab_p = q["labels"].cpu().numpy()
        assert np.array_equal(lab_g[:, :5], lab_p[:, :5]) and np.array_equal(lab_g[:, 5], ok_g)
        if j["rank"] is None:
            assert np.array_equal(rows_g, q["type2"].cpu().numpy()) and np.array_equal(ok_g, q["crc_ok"].cpu().numpy())
            continue
        listed = j["listed"]
        want, want_ok, want_rank, _ = E.decode_frames(tpsap, blk, words, types, listed, codes, D.BLK[tpsap][1], T)
        assert np.array_equal(j["rank"].cpu().numpy(), want_rank) and np.array_equal(ok_g, want_ok) and np.array_equal(rows_g, want), (tpsap, blk)
        t5, rc = frame_rows(golden, oracle, tpsap, blk, listed)
        b2, b_ok, b_rank = lb.decode_batch_list(tpsap, np.pad(t5, ((0, 0), (0, (-t5.shape[1]) % 4))), rc, T)
        assert np.array_equal(b_rank, want_rank) and np.array_equal(b_ok, want_ok) and np.array_equal(b2[:, :want.shape[1]], want), (tpsap, blk)
        assert (ok_g >= q["crc_ok"].cpu().numpy()).all()
        rescued += int((want_rank > 0).sum())
    assert rescued >= 10
    # ranked=False: exactly tetra_lmac_decode_frames_device
    again = jobs_for(False)
    lb.decode_frames_list_device(d_frames, d_types, again, T, frames_per_channel=nf, d_frame_bitnum=d_bitnum, d_time_rx=d_time, d_time=d_time, ranked=False)
    torch.cuda.synchronize()
    for a, q in zip(again, plain):
        assert torch.equal(a["type2"], q["type2"]) and torch.equal(a["crc_ok"], q["crc_ok"]) and torch.equal(a["labels"], q["labels"])
    bad = jobs_for(False)
    bad[4]["rank"] = torch.zeros(nf, dtype=torch.int32, device=dev)
    with pytest.raises(Exception):
        lb.decode_frames_list_device(d_frames, d_types, bad, T, frames_per_channel=nf, d_frame_bitnum=d_bitnum, d_time_rx=d_time, d_time=d_time)
    with pytest.raises(Exception):
        lb.decode_frames_list_device(d_frames, d_types, jobs_for(True), 9, frames_per_channel=nf, d_frame_bitnum=d_bitnum, d_time_rx=d_time, d_time=d_time)
    torch.cuda.synchronize()
