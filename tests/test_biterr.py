"""Channel bit-error counts of the coded blocks (include/ext/tetra_biterr.h) against the REFERENCE's own encoder: the decoded type-2 bits
go back through conv_enc_input -> get_punctured_rate -> block_interleave -> tetra_scramb_bits of oracle/_ref/libtetra_lmac_ref.so
(the transmit side of oracle/ref_binding.lmac_encode from type 2 on) and are held against the received row in numpy.  Nothing of the
product's code is in the expected values."""
import ctypes as C

import numpy as np
import pytest

from tests import chain_host as ch
from tests import soft_pipeline as sp
from tests.chain_gpu import device_bytes as _device_bytes, run_calls

CODED = (0, 1, 2, 4, 5)                   # SB1, SB2, NDB, SCH/HU, SCH/F
RATES = (0.0, 0.02, 0.05, 0.5)
PER_RATE = 60
SOFT_KINDS = {"sb1": 0, "sb2": 1, "ndb1": 2, "ndb2": 2, "schf": 5}


@pytest.fixture(scope="module")
def lref(ref):
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not built and /root/reference not present")
    return ref


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def reencode(ref, t, type2, code):
    """The type-5 bits a transmitter would send for the type-2 bits `type2` (all of them, tail included): the reference's primitives."""
    L = ref.lmac_lib()
    n345, n2, n1, a, _ = ref.BLK_PARAM[t]
    d = np.ascontiguousarray(type2, np.uint8)[:n2].copy()
    ces = np.zeros(64, np.uint8)
    L.conv_enc_init(_p(ces))
    mother = np.zeros(4 * n2, np.uint8)
    L.conv_enc_input(_p(ces), _p(d), n2, _p(mother))
    type3 = np.zeros(n345, np.uint8)
    L.get_punctured_rate(ref.RCPC_PUNCT_2_3, _p(mother), n345, _p(type3))
    type4 = np.zeros(n345, np.uint8)
    L.block_interleave(n345, a, _p(type3), _p(type4))
    L.tetra_scramb_bits(ref.SCRAMB_INIT if t == ref.TPSAP_T_SB1 else int(code) & 0xffffffff, _p(type4), n345)
    return type4


def count_hard(ref, t, row, code, type2, skip_tail=False, count_erasures=False):
    """(errors, compared) of the definition for a received byte row.  skip_tail / count_erasures: the two wrong variants the tests
    show they would notice (the tail bits taken as zero; an erasure taken as a received 1)."""
    n345, n2 = ref.BLK_PARAM[t][:2]
    code = ref.SCRAMB_INIT if t == ref.TPSAP_T_SB1 else int(code)
    d = np.array(type2[:n2], np.uint8)
    if skip_tail:
        d[n2 - 4:] = 0
    e = reencode(ref, t, d, code)
    seq = sp.scramb_seq(ref, code, n345)
    desc = np.asarray(row[:n345], np.uint8) ^ seq
    valid = np.ones(n345, bool) if count_erasures else desc != 0xff
    return int((valid & ((desc != 0) != ((e ^ seq) != 0))).sum()), int(valid.sum())


def count_soft(ref, t, soft5, code, type2):
    """... for received soft values (int8, positive = 0, as received: still scrambled)."""
    n345, n2 = ref.BLK_PARAM[t][:2]
    code = ref.SCRAMB_INIT if t == ref.TPSAP_T_SB1 else int(code)
    e = reencode(ref, t, type2, code)
    seq = sp.scramb_seq(ref, code, n345)
    v = np.where(seq != 0, -np.asarray(soft5[:n345], np.int16), np.asarray(soft5[:n345], np.int16))
    valid = v != 0
    return int((valid & ((v < 0) != ((e ^ seq) != 0))).sum()), int(valid.sum())


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


@pytest.fixture(scope="module")
def hard_rows(lref):
    """Per coded kind: PER_RATE encoded blocks per flip rate of RATES (plain 0 / 1 rows: 240), then 40 rows of the 0.05 kind in which
    a tenth of the positions are erasures (0xff after descrambling) and 40 in which set bits arrive as other byte values (2, 7, 0xfe
    after descrambling); the reference's decoding of every row and the definition's counts.  Computed once, read-only."""
    pool = {}
    for t in CODED:
        rng = np.random.default_rng(900 + t)
        n345, n2, n1, a, _ = lref.BLK_PARAM[t]
        n = PER_RATE * len(RATES) + 80
        si = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        if t == lref.TPSAP_T_SB1:
            si[:] = lref.SCRAMB_INIT
        rows = np.zeros((n, n345), np.uint8)
        flips = np.zeros(n, np.int64)
        rate = np.concatenate([np.repeat(RATES, PER_RATE), np.full(80, 0.05)])
        for b in range(n):
            f = rng.random(n345) < rate[b]
            flips[b] = f.sum()
            rows[b] = lref.lmac_encode(t, rng.integers(0, 2, n1).astype(np.uint8), int(si[b])) ^ f
            if b >= 240:
                seq = sp.scramb_seq(lref, int(si[b]), n345)
                pick = rng.random(n345) < 0.1
                if b < 280:
                    rows[b][pick] = 0xff ^ seq[pick]
                else:
                    pick &= (rows[b] ^ seq) != 0
                    rows[b][pick] = rng.choice(np.array([2, 7, 0xfe], np.uint8), int(pick.sum())) ^ seq[pick]
        want = np.zeros((n, n2), np.uint8)
        ok = np.zeros(n, np.int32)
        counts = np.zeros((n, 2), np.int64)
        for b in range(n):
            want[b], ok[b] = lref.lmac_decode(t, rows[b], si[b])
            counts[b] = count_hard(lref, t, rows[b], si[b], want[b])
        _freeze(rows, si, want, ok, counts, flips, rate)
        pool[t] = dict(rows=rows, si=si, want=want, ok=ok, counts=counts, flips=flips, rate=rate)
    return pool


def test_the_chosen_rows_tell_the_wrong_variants_apart(lref, hard_rows):
    """A count that takes the four tail bits as zero, or that counts erasures as received ones, differs from the definition on at least
    one of the rows used below, for every kind: the rows hold decoded blocks with a non-zero tail and rows with erasures."""
    for t in CODED:
        h = hard_rows[t]
        n2 = lref.BLK_PARAM[t][1]
        tails = int(h["want"][:, n2 - 4:].any(1).sum())
        assert tails >= 10, (t, tails)
        caught_tail = caught_erasure = 0
        for b in np.flatnonzero(h["want"][:, n2 - 4:].any(1)):
            caught_tail += count_hard(lref, t, h["rows"][b], h["si"][b], h["want"][b], skip_tail=True) != tuple(h["counts"][b])
        for b in range(240, 280):
            caught_erasure += count_hard(lref, t, h["rows"][b], h["si"][b], h["want"][b], count_erasures=True) != tuple(h["counts"][b])
        assert caught_tail >= 1 and caught_erasure == 40, (t, caught_tail, caught_erasure)


def test_definition_on_clean_and_lightly_damaged_rows(lref, hard_rows):
    """Rate 0: no errors and every position compared.  Rate 0.02: for blocks with a good CRC the count is the number of flips in at least
    90 % of them (the reference alone gives 95 % and more); on noise it never is."""
    for t in CODED:
        h = hard_rows[t]
        n345 = lref.BLK_PARAM[t][0]
        assert (h["counts"][:PER_RATE] == (0, n345)).all() and h["ok"][:PER_RATE].all()
        light = np.flatnonzero((h["rate"] == 0.02) & (h["ok"] == 1))[:PER_RATE]
        assert len(light) >= PER_RATE // 2
        assert (h["counts"][light, 0] == h["flips"][light]).mean() >= 0.9, t
        noise = slice(3 * PER_RATE, 4 * PER_RATE)
        assert (h["counts"][noise, 0] != h["flips"][noise]).all() and (h["counts"][noise, 0] < n345 // 4).all()


def test_lane_code_counts_equal_the_definition_on_byte_rows(lref, hard_rows):
    """reencode_errors (csrc/lmac_core.hpp) built for the host behind k_lmac_decode's front ends: the packed route (the three workgroups
    of plain 0 / 1 rows), the byte route (the workgroups with erasures and other bytes) and the byte route forced for every row give,
    row for row, the definition's errors and compared -- and the rows and verdicts the decoder gives without counting."""
    from tests.emul import lmac_biterr_emul_bind as E
    from tests.emul import lmac_emul_bind
    for t in CODED:
        h = hard_rows[t]
        rows = np.zeros((len(h["rows"]), 440), np.uint8)          # 8-byte aligned rows: the packed route is open
        rows[:, :h["rows"].shape[1]] = h["rows"]
        for route in (0, 1):
            out, ok, be, fast = E.decode_rows(t, rows, h["si"], route)
            assert fast == (192 if route == 0 else 0)
            assert np.array_equal(out, h["want"]) and np.array_equal(ok, h["ok"])
            plain, plain_ok, _ = lmac_emul_bind.decode_route(t, rows, h["si"], route)
            assert np.array_equal(out, plain) and np.array_equal(ok, plain_ok)
            err, cmp_ = E.split(be)
            assert np.array_equal(err, h["counts"][:, 0]) and np.array_equal(cmp_, h["counts"][:, 1]), (t, route)
        assert (h["counts"][240:280, 1] < lref.BLK_PARAM[t][0]).all()            # erasures are not compared


@pytest.fixture(scope="module")
def soft_rows(lref):
    """Per kind the soft route decodes: PER_RATE encoded blocks per flip rate as int8 soft values in [-31, 31] of random magnitude with
    zeros among them, the reference's soft decoding (tests/soft_pipeline.py) and the definition's counts."""
    pool = {}
    for kind, t in SOFT_KINDS.items():
        rng = np.random.default_rng(950 + len(pool))
        n345, n2, n1, a, _ = lref.BLK_PARAM[t]
        n = PER_RATE * len(RATES)
        si = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        if t == lref.TPSAP_T_SB1:
            si[:] = lref.SCRAMB_INIT
        rate = np.repeat(RATES, PER_RATE)
        soft = np.zeros((n, n345), np.int8)
        want = np.zeros((n, n2), np.uint8)
        ok = np.zeros(n, np.int32)
        counts = np.zeros((n, 2), np.int64)
        for b in range(n):
            bits = lref.lmac_encode(t, rng.integers(0, 2, n1).astype(np.uint8), int(si[b])) ^ (rng.random(n345) < rate[b])
            mag = rng.integers(1, 32, n345) * (rng.random(n345) >= 0.06)
            soft[b] = np.where(bits != 0, -mag, mag)
            want[b], ok[b] = sp.ref_soft_decode(lref, t, soft[b], int(si[b]))
            counts[b] = count_soft(lref, t, soft[b], si[b], want[b])
        assert (soft == 0).any(1).all() and soft.min() == -31 and soft.max() == 31
        _freeze(soft, si, want, ok, counts, rate)
        pool[kind] = dict(t=t, soft=soft, si=si, want=want, ok=ok, counts=counts, rate=rate)
    return pool


def test_lane_code_counts_equal_the_definition_on_soft_values(lref, soft_rows):
    """The same lane function behind k_lmac_frames_soft's front end (values staged from a ring, descrambled by sign): errors and compared
    equal the definition on every row, zeros are not compared, and clean rows count no error."""
    from tests.emul import lmac_biterr_emul_bind as E
    for kind, s in soft_rows.items():
        out, ok, be = E.decode_soft_rows(kind, s["soft"], None if s["t"] == 0 else s["si"])
        assert np.array_equal(out, s["want"]) and np.array_equal(ok, s["ok"]), kind
        err, cmp_ = E.split(be)
        assert np.array_equal(err, s["counts"][:, 0]) and np.array_equal(cmp_, s["counts"][:, 1]), kind
        assert np.array_equal(cmp_, (s["soft"] != 0).sum(1)) and (err[:PER_RATE] == 0).all() and s["ok"][:PER_RATE].all()
        assert (err[3 * PER_RATE:] > 0).all()


def test_lane_code_counts_from_packed_frames(lref, oracle):
    """... and behind k_lmac_frames' front end (the block cut out of a packed frame): the listed frames of every kind -- a few of another
    burst type among them, the all-zero block -- count what the definition gives for the demultiplexed row."""
    from tests.emul import lmac_biterr_emul_bind as E
    from tests.test_lmac import FRAME_KINDS, make_frames
    frames, packed, types, codes = make_frames(lref, oracle, 120, 41)
    for tpsap, blk, train in FRAME_KINDS[:5]:
        carrying = [r for r in range(len(types)) if types[r] == train]
        listed = np.array(carrying + [r for r in range(len(types)) if types[r] != train][:5], np.int32)
        n345, n2 = lref.BLK_PARAM[tpsap][:2]
        out, ok, be = E.decode_frames(tpsap, blk, packed, types, listed, None if tpsap == 0 else codes, n2)
        err, cmp_ = E.split(be)
        for j, r in enumerate(listed):
            row = oracle.bsync_demux(frames[r], int(types[r]), tpsap, blk) if types[r] >= 0 else np.zeros(0, np.uint8)
            t5 = np.zeros(n345, np.uint8)
            t5[:row.size] = row
            want, want_ok = lref.lmac_decode(tpsap, t5, codes[r])
            assert np.array_equal(out[j], want) and ok[j] == want_ok
            assert (err[j], cmp_[j]) == count_hard(lref, tpsap, t5, codes[r], want), (tpsap, blk, j)
        assert (cmp_ == n345).all() and (err[:len(carrying)] == 0).any() and (err > 0).any()


def test_extension_header_is_exported_and_bound(pkg):
    """tests/test_abi.py's rule for the extension header include/ext/tetra_biterr.h: every function it declares is exported by the library and
    has an entry with as many parameters in a binding module's BITERR_ABI table; the header compiles as C."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = os.path.join(root, "include", "ext", "tetra_biterr.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): [a for a in " ".join(m.group(2).split()).split(",")] for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    tables = {**pkg.lmac_binding.BITERR_ABI, **pkg.rx_binding.BITERR_ABI}
    assert len(decls) == 6 and set(decls) == set(tables)
    L = pkg.load_library()
    pkg.lmac_binding._lib(), pkg.rx_binding._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        assert len(tables[name][1]) == len(params) == len(fn.argtypes), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    assert C.sizeof(pkg.rx_binding.Link) == 24
    assert "TETRA_RX_FLAG_BITERR = 32" in open(os.path.join(root, "include", "tetra_rx.h")).read() and pkg.rx_binding.FLAG_BITERR == 32


def test_lane_code_counts_are_clean_under_asan_and_ubsan():
    """The same host build as a stand-alone program (tests/san/san_biterr.cpp) under AddressSanitizer and UBSan, on exact-size heap
    buffers: both routes of the byte rows at a ragged workgroup, frames of every burst type, soft values from rings that wrap."""
    import os
    import subprocess
    from tests.test_sanitizers import ENV, FLAGS, SAN, _stale
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(SAN, "san_biterr")
    srcs = [os.path.join(SAN, "san_biterr.cpp"), os.path.join(root, "tests", "emul", "lmac_biterr_emul.cpp")]
    deps = srcs + [os.path.join(root, "tests", "emul", "lmac_lane_io.hpp")] + \
        [os.path.join(root, "sdrpp-tetra-demodulator_amd", "csrc", f) for f in ("lmac_core.hpp", "soft_core.hpp", "demux_core.hpp")]
    if _stale(exe, deps):
        subprocess.run(["g++", "-std=c++17", "-Wall"] + FLAGS + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "san_biterr: ok" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _dev(pkg):
    import torch
    return torch, torch.device("cuda", 0)


def _u32(torch, a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)


SENTINEL = 0x5a5a5a5a


@pytest.mark.gpu
@pytest.mark.parametrize("t", CODED)
def test_gpu_byte_rows_count_the_definition(pkg, lref, hard_rows, t):
    """tetra_lmac_decode_counted_biterr_device at the 64-row workgroup edge (1, 63, 64, 65, 130 rows), tight and padded input rows, the
    packed route and the byte route forced, rows of plain bits and rows with erasures and other bytes: the counts are the definition's,
    rows and verdicts are byte for byte those of tetra_lmac_decode_counted_device on the same input, and with a device-side row count
    below the capacity the entries past it keep their sentinel."""
    torch, dev = _dev(pkg)
    lb = pkg.lmac_binding
    h = hard_rows[t]
    n345, n2 = lref.BLK_PARAM[t][:2]
    ost = lb.out_stride_for(t)
    for first, n in ((0, 1), (0, 63), (0, 64), (0, 65), (190, 130)):          # (the last run crosses from plain rows into erasures)
        sel = slice(first, first + n)
        for stride in (n345, n345 + (-n345) % 8 + 8):
            rows = np.zeros((n, stride), np.uint8)
            rows[:, :n345] = h["rows"][sel]
            d_rows = torch.from_numpy(rows).to(dev)
            d_si = None if t == 0 else _u32(torch, h["si"][sel], dev)
            for forced in (False, True):
                t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
                t2p = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
                ok = torch.full((n,), -3, dtype=torch.int32, device=dev)
                okp = torch.full((n,), -3, dtype=torch.int32, device=dev)
                be = _u32(torch, np.full(n, SENTINEL), dev)
                lb.force_byte_route(forced)
                try:
                    lb.decode_counted_biterr_device(t, d_rows, n, None, stride, d_si, None, t2, ost, ok, be)
                    lb.decode_counted_device(t, d_rows, n, None, stride, d_si, None, t2p, ost, okp)
                    torch.cuda.synchronize()
                finally:
                    lb.force_byte_route(False)
                assert torch.equal(t2, t2p) and torch.equal(ok, okp)
                assert np.array_equal(t2.cpu().numpy()[:, :n2], h["want"][sel]) and np.array_equal(ok.cpu().numpy(), h["ok"][sel])
                err, cmp_ = lb.split_biterr(be.cpu().numpy())
                assert np.array_equal(err, h["counts"][sel, 0]) and np.array_equal(cmp_, h["counts"][sel, 1]), (t, n, stride, forced)
    # a device-side count below the capacity
    n, have = 130, 70
    rows = np.ascontiguousarray(h["rows"][:n])
    d_rows, d_si = torch.from_numpy(rows).to(dev), (None if t == 0 else _u32(torch, h["si"][:n], dev))
    t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
    ok = torch.full((n,), -3, dtype=torch.int32, device=dev)
    be = _u32(torch, np.full(n, SENTINEL), dev)
    lb.decode_counted_biterr_device(t, d_rows, n, torch.tensor([have], dtype=torch.int32, device=dev), n345, d_si, None, t2, ost, ok, be)
    torch.cuda.synchronize()
    got = be.cpu().numpy().view(np.uint32)
    assert (got[have:] == SENTINEL).all() and (ok[have:] == -3).all() and (t2[have:] == 7).all()
    err, cmp_ = lb.split_biterr(got[:have])
    assert np.array_equal(err, h["counts"][:have, 0]) and np.array_equal(cmp_, h["counts"][:have, 1])


@pytest.mark.gpu
def test_gpu_byte_rows_host_entry_and_argument_errors(pkg, lref, hard_rows):
    """tetra_lmac_decode_batch_biterr (host pointers) counts the same; a count array for the AACH is TETRA_ERR_ARG, a misaligned one
    TETRA_ERR_ALIGN, and NULL is the existing entry point."""
    torch, dev = _dev(pkg)
    lb = pkg.lmac_binding
    h = hard_rows[5]
    t2, ok, be = lb.decode_batch_biterr(5, h["rows"][200:300], h["si"][200:300])
    plain, plain_ok = lb.decode_batch(5, h["rows"][200:300], h["si"][200:300])
    assert np.array_equal(t2, plain) and np.array_equal(ok, plain_ok) and np.array_equal(ok, h["ok"][200:300])
    err, cmp_ = lb.split_biterr(be)
    assert np.array_equal(err, h["counts"][200:300, 0]) and np.array_equal(cmp_, h["counts"][200:300, 1])
    L = pkg.binding.load_library()
    ERR_ARG, ERR_ALIGN = -1, -7                                          # include/tetra_demod.h
    rows = torch.zeros((4, 432), dtype=torch.uint8, device=dev)
    si = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.zeros((4, 288), dtype=torch.uint8, device=dev)
    okd = torch.zeros(4, dtype=torch.int32, device=dev)
    bed = torch.zeros(8, dtype=torch.int32, device=dev)
    f = L.tetra_lmac_decode_counted_biterr_device
    assert f(3, rows.data_ptr(), 4, None, 432, si.data_ptr(), None, out.data_ptr(), 288, okd.data_ptr(), bed.data_ptr(), None) == ERR_ARG
    assert f(3, rows.data_ptr(), 4, None, 432, si.data_ptr(), None, out.data_ptr(), 288, okd.data_ptr(), None, None) == 0
    assert f(5, rows.data_ptr(), 4, None, 432, si.data_ptr(), None, out.data_ptr(), 288, okd.data_ptr(), bed.data_ptr() + 2, None) == ERR_ALIGN
    assert f(5, rows.data_ptr(), 4, None, 432, si.data_ptr(), None, out.data_ptr(), 288, okd.data_ptr(), None, None) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_frames_count_like_the_byte_rows(pkg, lref, oracle):
    """tetra_lmac_decode_frames_biterr_device, every kind in one launch, some jobs with a count array and some without, listed frames of
    another burst type among them: the counts equal the byte-row entry's on the demultiplexed rows (and the definition), rows, verdicts
    and labels are those of tetra_lmac_decode_frames_device, rows past a job's count keep their sentinel, and a count array on a BBK
    job is TETRA_ERR_ARG."""
    torch, dev = _dev(pkg)
    from tests.test_lmac import make_frames
    lb = pkg.lmac_binding
    F, n = 16, 96
    frames, packed, types, codes = make_frames(lref, oracle, n, 57)
    d_fr, d_ft, d_codes = _u32(torch, packed, dev), torch.from_numpy(types).to(dev), _u32(torch, codes, dev)
    bitnum = torch.arange(n, dtype=torch.int32, device=dev) * 510 + 7
    t_rx = torch.arange(n, dtype=torch.int32, device=dev) + 1000
    t_af = torch.arange(n, dtype=torch.int32, device=dev) + 5000
    # (tpsap, blk, carrying burst type, counts?)
    kinds = ((5, 0, 0, True), (1, 2, 3, True), (2, 1, 1, False), (2, 2, 1, True), (3, 0, None, False), (0, 1, 3, True))
    jobs, plain_jobs, lists = [], [], []
    for tpsap, blk, train, counts in kinds:
        carrying = [r for r in range(n) if (types[r] == train if train is not None else types[r] in (0, 1, 3))]
        listed = np.array(carrying + [r for r in range(n) if r not in carrying and types[r] >= 0][:3], np.int32)
        lists.append(listed)
        n2 = 32 if tpsap == 3 else lref.BLK_PARAM[tpsap][1]
        cap = len(listed) + 5

        def outputs():
            return dict(type2=torch.full((cap, n2 + 8), 5, dtype=torch.uint8, device=dev), crc_ok=torch.full((cap,), -3, dtype=torch.int32, device=dev),
                        labels=torch.full((cap, 6), -1, dtype=torch.int32, device=dev))
        d_list = torch.from_numpy(np.concatenate([listed, np.zeros(5, np.int32)])).to(dev)
        base = dict(type=tpsap, blk_num=blk, row_frame=d_list, n_rows=torch.tensor([len(listed)], dtype=torch.int32, device=dev), max_rows=cap,
                    out_stride=n2 + 8, frame_scramb=None if tpsap == 0 else d_codes)
        jobs.append(dict(base, **outputs(), biterr=_u32(torch, np.full(cap, SENTINEL), dev) if counts else None))
        plain_jobs.append(dict(base, **outputs()))
    lb.decode_frames_biterr_device(d_fr, d_ft, jobs, F, bitnum, t_rx, t_af)
    lb.decode_frames_device(d_fr, d_ft, plain_jobs, F, bitnum, t_rx, t_af)
    again = [dict(j, **{k: torch.full_like(j[k], 9) for k in ("type2", "crc_ok", "labels")}) for j in plain_jobs]
    lb.decode_frames_biterr_device(d_fr, d_ft, again, F, bitnum, t_rx, t_af, counted=False)          # a NULL array
    torch.cuda.synchronize()
    some_errors = 0
    for (tpsap, blk, train, counts), listed, j, pj, aj in zip(kinds, lists, jobs, plain_jobs, again):
        n2 = 32 if tpsap == 3 else lref.BLK_PARAM[tpsap][1]
        for k in ("type2", "crc_ok", "labels"):
            assert torch.equal(j[k], pj[k]), (tpsap, blk, k)
            a_used, p_used = aj[k][:len(listed)], pj[k][:len(listed)]
            if k == "type2":                                      # (the rows' padding keeps each run's own fill)
                a_used, p_used = a_used[:, :n2], p_used[:, :n2]
            assert torch.equal(a_used, p_used) and (aj[k][len(listed):] == 9).all()
        if not counts:
            continue
        n345 = lref.BLK_PARAM[tpsap][0]
        rows = np.zeros((len(listed), n345), np.uint8)
        for i, r in enumerate(listed):
            row = oracle.bsync_demux(frames[r], int(types[r]), tpsap, blk)
            rows[i, :row.size] = row
        t2, ok, be = lb.decode_batch_biterr(tpsap, rows, None if tpsap == 0 else codes[listed])
        got = j["biterr"].cpu().numpy().view(np.uint32)
        assert (got[len(listed):] == SENTINEL).all()
        assert np.array_equal(got[:len(listed)], be), (tpsap, blk)
        assert np.array_equal(j["type2"].cpu().numpy()[:len(listed), :t2.shape[1]], t2) and np.array_equal(j["crc_ok"].cpu().numpy()[:len(listed)], ok)
        err, cmp_ = lb.split_biterr(be)
        for i, r in enumerate(listed):
            assert (err[i], cmp_[i]) == count_hard(lref, tpsap, rows[i], codes[r], t2[i]), (tpsap, blk, i)
        some_errors += int((err > 0).sum())
    assert some_errors > 10
    # the same launch with the AACH job decoded by its Reed-Muller code (TETRA_LMAC_JOB_RM3014): the counting instantiation of that
    # kernel gives the counts of the launch above and the rows, verdicts and labels of the launch without counts
    def fresh(js, counted):
        out = []
        for j in js:
            o = dict(j, type=j["type"] | (lb.JOB_RM3014 if j["type"] == 3 else 0), **{k: torch.full_like(j[k], 5) for k in ("type2", "crc_ok", "labels")})
            if counted and j.get("biterr") is not None:
                o["biterr"] = _u32(torch, np.full(j["biterr"].numel(), SENTINEL), dev)
            out.append(o)
        return out
    rm_jobs, rm_plain = fresh(jobs, True), fresh(plain_jobs, False)
    lb.decode_frames_biterr_device(d_fr, d_ft, rm_jobs, F, bitnum, t_rx, t_af)
    lb.decode_frames_device(d_fr, d_ft, rm_plain, F, bitnum, t_rx, t_af)
    torch.cuda.synchronize()
    for j, rj, rp in zip(jobs, rm_jobs, rm_plain):
        assert all(torch.equal(rj[k], rp[k]) for k in ("type2", "crc_ok", "labels"))
        assert (j.get("biterr") is None) == (rj.get("biterr") is None) and (j.get("biterr") is None or torch.equal(j["biterr"], rj["biterr"]))
    assert not torch.equal(rm_jobs[4]["type2"], jobs[4]["type2"])         # (the AACH rows do carry the decoder's distance byte)
    bbk = [dict(jobs[4], biterr=jobs[0]["biterr"])]
    with pytest.raises(pkg.TetraDemodError) as e:
        lb.decode_frames_biterr_device(d_fr, d_ft, bbk, F, bitnum, t_rx, t_af)
    assert e.value.status == -1                                           # TETRA_ERR_ARG
    with pytest.raises(pkg.TetraDemodError) as e:                         # a count array that is not 4-byte aligned
        lb.decode_frames_biterr_device(d_fr, d_ft, [dict(jobs[0], biterr=jobs[0]["biterr"].data_ptr() + 2)], F, bitnum, t_rx, t_af)
    assert e.value.status == -7                                           # TETRA_ERR_ALIGN
    torch.cuda.synchronize()


# ---- GPU: the receive chain (TETRA_RX_FLAG_BITERR) ---------------------------------------------------------------------------------------
CH_SAMPLES, CH_CUT, CH_SLOTS = 18000, 9000, 36
CH_ESN0 = (None, 11.0, 11.5)                   # three coded downlinks: a clean one and two near 11 dB; channel 3 is noise only
CODED_KINDS = ch.CODED_KINDS
ERR_UNSUPPORTED = -2                           # include/tetra_demod.h


@pytest.fixture(scope="module")
def chain_iq(synth):
    rows = []
    for c, esn0 in enumerate(CH_ESN0):
        tx = synth.gen_downlink(CH_SLOTS, 7100 + c, cell=(200 + c, 3000 + c, 9 + c))
        rows.append(synth.gen_channel(CH_SAMPLES, 7200 + c, bits=tx[0], esn0_db=esn0)[0])
    rng = np.random.default_rng(7300)
    rows.append((rng.normal(0, 0.7, CH_SAMPLES) + 1j * rng.normal(0, 0.7, CH_SAMPLES)).astype(np.complex64))
    iq = np.stack(rows).astype(np.complex64)
    iq.flags.writeable = False
    return iq


def _run_chain(pkg, iq, flags, after=None):
    """the stream in two calls through one handle -> per call {kind: (blocks, type1)}, the channels' bits of both calls, and after(rx)"""
    import torch
    R = pkg.rx_binding
    calls = []

    def per_call(rx, i, s):
        if i == 0 and flags & R.FLAG_BITERR:
            assert all(len(rx.fetch_biterr(k, which=1)[0]) == 0 for k in CODED_KINDS)          # no previous call yet
        calls.append({k: rx.fetch(k) for k in range(R.N_KINDS)})
        if flags & R.FLAG_BITERR:
            calls[-1]["biterr"] = {k: rx.fetch_biterr(k) for k in CODED_KINDS}
            for k in CODED_KINDS:          # the same rows where they are, beside rows_device's; and a buffer that is too small
                n = len(calls[-1][k][0])
                if n:
                    words = _device_bytes(torch, rx.biterr_device(k, 0, s), (n,), "<i4").cpu().numpy().astype(np.int64) & 0xffffffff
                    assert np.array_equal(words & 0xffff, calls[-1]["biterr"][k][0]) and np.array_equal(words >> 16, calls[-1]["biterr"][k][1])
                    _, _, _, pn_rows = rx.rows_device(k, 0, s)
                    assert int(_device_bytes(torch, pn_rows, (1,), "<i4").cpu().numpy()[0]) == n
                    got, small = C.c_int(0), np.zeros(max(n - 1, 1), np.uint32)
                    assert rx._lib.tetra_rx_fetch_biterr(rx._h, 0, k, small.ctypes.data, n - 1, C.byref(got)) == -6 and got.value == n      # TETRA_ERR_SIZE

    bits, cells, extra = run_calls(pkg, iq, (0, CH_CUT, CH_SAMPLES), flags, per_call, after=after)
    return calls, bits, cells, extra


def _codes_in_force(ref, calls, n_channels):
    """per channel the (bit number, scrambling code) of every SB1 with a good CRC, in stream order: what tp_sap_udata_ind's SB1 case sets"""
    out = [[] for _ in range(n_channels)]
    for call in calls:
        blocks, t1 = call[ch.KIND_SB1]
        for b, t in zip(blocks, t1):
            if b["crc_ok"]:
                out[int(b["channel"])].append((int(b["bitnum"]), ref.scramb_get_init(*ch.sync_pdu_fields(t)[:3])))
    return out


def _expected_counts(ref, calls, bits, soft=None):
    """The definition on every coded row of both calls, from the chain's own bits (soft = None) or from soft values per channel: the
    row's type-5 block is cut at its label's bit number with chain_host's pieces, decoded by the reference under the code in force, and
    counted.  -> per call {kind: (errors, compared)}; the reference's type-1 bits and verdicts are checked on the way."""
    codes = _codes_in_force(ref, calls, len(bits))
    out = []
    for call in calls:
        want = {}
        for k in CODED_KINDS:
            tpsap, pieces = ch.BY_KIND[k].tpsap, ch.BY_KIND[k].pieces
            blocks, t1 = call[k]
            v = np.zeros((len(blocks), 2), np.int64)
            for j, b in enumerate(blocks):
                c, bn = int(b["channel"]), int(b["bitnum"])
                code = ([0] + [cd for at, cd in codes[c] if at <= bn])[-1]
                src = bits[c] if soft is None else soft[c]
                t5 = ch.cut(src, bn, pieces)
                if soft is None:
                    t2, ok = ref.lmac_decode(tpsap, t5, code)
                    v[j] = count_hard(ref, tpsap, t5, code, t2)
                else:
                    t2, ok = sp.ref_soft_decode(ref, tpsap, t5, code)
                    v[j] = count_soft(ref, tpsap, t5, code, t2)
                assert ok == b["crc_ok"] and np.array_equal(t2[:t1.shape[1]], t1[j]), (k, j)
            want[k] = v
        out.append(want)
    return out


def _link_sums(calls, n_channels):
    want = [dict(bits=0, bit_errors=0, blocks=0, blocks_crc_bad=0) for _ in range(n_channels)]
    for call in calls:
        for k in CODED_KINDS:
            blocks = call[k][0]
            err, cmp_ = call["biterr"][k]
            for b, e, n in zip(blocks, err, cmp_):
                w = want[int(b["channel"])]
                w["blocks"] += 1
                if b["crc_ok"]:
                    w["bits"] += int(n)
                    w["bit_errors"] += int(e)
                else:
                    w["blocks_crc_bad"] += 1
    return want


@pytest.fixture(scope="module")
def chain_plain(pkg, chain_iq):
    """the same stream through handles without the flag: hard on two streams, soft, hard on one stream"""
    R = pkg.rx_binding
    return {f: _run_chain(pkg, chain_iq, f) for f in (0, R.FLAG_SOFT, R.FLAG_ONE_STREAM)}


@pytest.mark.gpu
@pytest.mark.parametrize("route", ("hard", "soft", "one_stream"))
def test_gpu_chain_counts_links_and_resets(pkg, lref, oracle, chain_iq, chain_plain, route):
    """TETRA_RX_FLAG_BITERR alone, with TETRA_RX_FLAG_SOFT and with TETRA_RX_FLAG_ONE_STREAM, a stream of three coded downlinks (one
    clean, two near 11 dB) and a noise channel in two calls: blocks, type-1 bits, AACH rows and cells are those of the same handle without
    the flag; fetch_biterr is the definition on the chain's own frames (soft: on the quantised oracle symbols through the reference's soft
    decoder); links() is the sum over both calls; reset_channels([1]) zeroes channel 1's link only and reset() all of them."""
    R = pkg.rx_binding
    base = {"hard": 0, "soft": R.FLAG_SOFT, "one_stream": R.FLAG_ONE_STREAM}[route]
    C = chain_iq.shape[0]

    def after(rx):
        links = rx.links()
        rx.reset_channels([1])
        one = rx.links()
        rx.reset()
        return links, one, rx.links()
    calls, bits, cells, (links, after_one, after_all) = _run_chain(pkg, chain_iq, base | R.FLAG_BITERR, after)
    plain_calls, plain_bits, plain_cells, _ = chain_plain[base]
    for call, plain in zip(calls, plain_calls):
        for k in range(R.N_KINDS):
            assert np.array_equal(call[k][0], plain[k][0]) and np.array_equal(call[k][1], plain[k][1]), k
    assert cells == plain_cells and all(np.array_equal(a, b) for a, b in zip(bits, plain_bits))
    soft = None
    if route == "soft":
        _, nb, sym, _ = oracle.process_batch(np.array(chain_iq), want_sym=True)
        soft = [sp.quantise_np(sym[c][:nb[c] // 2]) for c in range(C)]
    want = _expected_counts(lref, calls, bits, soft)
    rows = errors = 0
    for call, w in zip(calls, want):
        for k in CODED_KINDS:
            err, cmp_ = call["biterr"][k]
            assert np.array_equal(err, w[k][:, 0]) and np.array_equal(cmp_, w[k][:, 1]), (route, k)
            rows += len(err)
            errors += int(err.sum())
    assert rows >= 60 and errors > 0
    assert links == _link_sums(calls, C)
    assert links[0]["blocks"] > 20 and links[1]["bit_errors"] > links[0]["bit_errors"] and sum(l["blocks_crc_bad"] for l in links[1:]) > 0
    zero = dict(bits=0, bit_errors=0, blocks=0, blocks_crc_bad=0)
    assert after_one == [zero if c == 1 else links[c] for c in range(C)]
    assert after_all == [zero] * C


@pytest.mark.gpu
def test_gpu_chain_without_the_flag_refuses(pkg, chain_iq):
    R = pkg.rx_binding
    assert R.FLAG_BITERR == 32
    rx = pkg.RxChain(2, 4000)
    try:
        for f in (lambda: rx.fetch_biterr(R.KIND_SCH_F), rx.links, lambda: rx.biterr_device(R.KIND_SCH_F)):
            with pytest.raises(pkg.TetraDemodError) as e:
                f()
            assert e.value.status == ERR_UNSUPPORTED
    finally:
        rx.close()
    for bad in (4, 16, 64):                                # still no flags
        with pytest.raises(pkg.TetraDemodError):
            pkg.RxChain(2, 4000, flags=R.FLAG_BITERR | bad)
    rx = pkg.RxChain(2, 4000, flags=R.FLAG_BITERR, kinds=1 << R.KIND_SCH_F)
    try:
        for k in (R.KIND_BBK, R.KIND_SB2):                 # the AACH has no count; SB2 is not decoded by this handle
            with pytest.raises(pkg.TetraDemodError) as e:
                rx.fetch_biterr(k)
            assert e.value.status == ERR_UNSUPPORTED
        assert len(rx.fetch_biterr(R.KIND_SCH_F)[0]) == 0 and len(rx.fetch_biterr(R.KIND_SB1)[0]) == 0
    finally:
        rx.close()


@pytest.mark.gpu
def test_gpu_wideband_links_and_retune(pkg, synth):
    """The wideband handle with the flag in cfg.rx.flags (the smallest configuration of tests/test_wbrx.py): links() of the carrier slots
    are the sums over the chain's own rows, and after a retune the moved slot's link is zero while the others keep theirs."""
    import torch
    from tests.test_wbrx import BINS_SMALL, CARRIERS_SMALL, D_SMALL, M_SMALL, _capture
    R = pkg.rx_binding
    x, _, _ = _capture(torch, synth, M_SMALL, CARRIERS_SMALL, 24)
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=x.shape[0], flags=R.FLAG_BITERR)
    try:
        s = torch.cuda.current_stream()
        wb.process_device(x, x.shape[0], s)
        call = {k: wb.rx.fetch(k) for k in range(R.N_KINDS)}
        call["biterr"] = {k: wb.rx.fetch_biterr(k) for k in CODED_KINDS}
        links = wb.links()
        assert links == _link_sums([call], len(BINS_SMALL)) and all(l["blocks"] > 0 for l in links)
        moved = list(BINS_SMALL)
        moved[2] = 9
        wb.retune(moved, s)
        zero = dict(bits=0, bit_errors=0, blocks=0, blocks_crc_bad=0)
        assert wb.links() == [zero if c == 2 else links[c] for c in range(len(BINS_SMALL))]
    finally:
        wb.close()


@pytest.mark.gpu
def test_gpu_host_banks_fetch_bit_errors_and_links(pkg, synth, tmp_path):
    """TetraRxBank::fetchBitErrors / links and the TetraRxMultiBank concatenation (host/tetra_rx_bank.h), 3 shards on one GPU against one
    bank of all channels: the same counts row for row, the same link figures in channel order, and those are the sums of the rows; a plain
    C++ driver (tests/host/test_biterr_bank.cpp)."""
    import os
    import subprocess
    from tests.chain_host import noisy_batch as _noisy_batch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pk = os.path.join(root, "sdrpp-tetra-demodulator_amd")
    pkg.build.build()
    exe = os.path.join(root, "tests", "host", "test_biterr_bank")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(root, "include"), "-I", os.path.join(pk, "host"),
                    os.path.join(root, "tests", "host", "test_biterr_bank.cpp"), "-L", pk, "-ltetra_demod_hip", "-Wl,-rpath," + pk, "-o", exe], check=True)
    Cn, calls, nslots = 7, 2, 32
    N = nslots * 510 // calls
    _, _, iq = _noisy_batch(synth, Cn, nslots, N * calls, 8950)
    f = tmp_path / "iq.bin"
    with open(f, "wb") as fh:
        for k in range(calls):
            fh.write(np.ascontiguousarray(iq[:, k * N:(k + 1) * N]).astype(np.complex64).tobytes())
    r = subprocess.run([exe, str(Cn), str(N), str(calls), str(f), "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_biterr_bank: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[2]) > 100 and int(r.stdout.split()[4]) > 0
