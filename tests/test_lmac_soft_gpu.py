"""The soft frame decoder's DEVICE build on chosen rings (include/ext/tetra_soft.h: tetra_lmac_decode_frames_soft_device, the public
entry to k_lmac_frames_soft, its counting instantiation and the list rescue with the soft front end), against the REFERENCE's own chain
-- sign-descramble -> block_deinterleave -> tetra_rcpc_depunct -> conv_cch_decode -> crc16_ccitt_bits (tests/soft_pipeline.ref_soft_decode
on oracle/_ref) --, the counts' definition (tests/list_definition.count_errors) and the list decoding's (tests/list_definition.list_decode).
Everything is integer: every comparison is exact.

The planted rows are tests/soft_pipeline.soft_rows_for's (clean, noisy and random rows, the int16 bound's all-(+-Q) and alternating rows,
ties, the all-zero row) and the soft rows of tests/golden/list_golden.npz; they are made again from their seeds here.  Where oracle/_ref
is built the expected values come from the reference, elsewhere from tests/golden/lmac_soft_golden.npz, which a CPU test holds against
the reference whenever that is at hand."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import list_definition as D
from tests import soft_pipeline as sp
from tests.golden import make_lmac_soft_golden as G
from tests.test_list_decode import for_T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = G.KINDS
FPC = 7                                  # frames per channel: channel = frame / 7
SENTINEL = 0x5a5a5a5a
ERR_ARG = -1                             # include/tetra_demod.h
ZERO_ROWS = slice(88, 92)                # soft_rows_for: the all-zero row under codes 0, 3, 0xffffffff and a random one
BOUND_ROWS = slice(72, 88)               # ... all +Q, all -Q and the two alternating rows under the same four codes


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return d


def _have_ref():
    from oracle import ref_binding
    return ref_binding.available() and ref_binding.lmac_available()


@pytest.fixture(scope="module")
def want():
    """Per kind, read-only: the planted rows and codes, the reference's bits, verdicts and counts on them, the definition's list result
    with eight candidates on them; the same for the list rows under list_*.  From oracle/_ref where it is built, else the fixture."""
    from oracle import ref_binding
    from_ref = _have_ref()
    g = G.make(ref_binding) if from_ref else np.load(G.PATH)
    print("expected values from", "oracle/_ref" if from_ref else "tests/golden/lmac_soft_golden.npz")
    pool = {"source": "oracle/_ref" if from_ref else "fixture"}
    for kind in KINDS:
        t, n2 = sp.REF_TPSAP[kind], sp.TYPE2_BITS[kind]
        e = {"t": t}
        for pre, (rows, codes) in (("", G.planted(kind)), ("list_", G.list_rows(kind))):
            assert np.array_equal(G.checksum(rows, codes), g[kind + "_" + pre + "sum"]), (kind, pre)      # the rows the answers belong to
            e[pre + "rows"], e[pre + "codes"] = rows, codes
            e[pre + "t2"], e[pre + "ok"] = np.unpackbits(g[kind + "_" + pre + "t2"], axis=1)[:, :n2], g[kind + "_" + pre + "ok"]
            e[pre + "def"] = _freeze(D.list_decode(t, D.soft_values(t, rows, codes), 8, D.START_SOFT))
        e["biterr"], e["list_rank"] = g[kind + "_biterr"], g[kind + "_list_rank"]
        pool[kind] = _freeze(e)
    return pool


def counts_after(e, pre, idx, out):
    """errors | compared << 16 of the definition for rows idx of a pool and the bits they ended up with"""
    return G.counts_of(e["t"], e[pre + "rows"][idx], e[pre + "codes"][idx], out)


# ---- CPU: the inputs mean something, the fixture is the reference's, the host build agrees ---------------------------------------------
def test_planted_rows_hold_every_case_by_the_reference_alone(want):
    for kind in KINDS:
        e = want[kind]
        rows, codes, ok = e["rows"], e["codes"], e["ok"]
        assert len(rows) == 100 and ok.sum() >= 12 and (ok == 0).sum() >= 1, kind
        n345 = rows.shape[1]
        alt = np.where(np.arange(n345) % 2 == 0, sp.Q, -sp.Q)
        for k, r in enumerate((np.full(n345, sp.Q), np.full(n345, -sp.Q), alt, -alt, np.zeros(n345))):
            four = slice(BOUND_ROWS.start + 4 * k, BOUND_ROWS.start + 4 * k + 4)
            assert (rows[four] == r).all() and list(codes[four][:3]) == [0, 3, 0xffffffff] and codes[four][3] not in (0, 3, 0xffffffff), (kind, k)
        assert (rows[ZERO_ROWS] == 0).all() and (e["t2"][ZERO_ROWS] == 0).all() and (ok[ZERO_ROWS] == 0).all()
        assert np.abs(rows).max() == sp.Q == 31
        # the definition's maximum-likelihood path is the reference's decoding, on the planted rows and on the list rows
        for pre in ("", "list_"):
            assert np.array_equal(e[pre + "def"]["ml"], e[pre + "t2"]) and np.array_equal(e[pre + "def"]["ml_ok"], e[pre + "ok"]), (kind, pre)
        rank = e["list_def"]["rank"]
        assert np.array_equal(rank, e["list_rank"]) and len(rank) == 64
        assert (rank == 0).sum() >= 10 and (rank >= 1).sum() >= 5 and (rank == -1).sum() >= 3, kind
        # counts: a clean full-scale codeword compares every position and differs nowhere; the all-zero row compares none
        assert e["biterr"][0] == n345 << 16 and (e["biterr"][ZERO_ROWS] == 0).all()


def test_fixture_is_the_reference(want):
    """tests/golden/lmac_soft_golden.npz is what tests/golden/make_lmac_soft_golden.py makes from oracle/_ref; the planted rows made with
    the reference's encoder are those made with tests/list_definition.encode."""
    from oracle import ref_binding
    if not _have_ref():
        pytest.skip("oracle/_ref not built and the reference not present")
    again, g = G.make(ref_binding), np.load(G.PATH)
    assert set(again) == set(g.files)
    for k in again:
        assert np.array_equal(again[k], g[k]), k
    for kind in KINDS:
        rows, codes = G.planted(kind, ref_binding)
        assert np.array_equal(rows, want[kind]["rows"]) and np.array_equal(codes, want[kind]["codes"]), kind


@pytest.mark.parametrize("kind", KINDS)
def test_host_emulation_equals_the_reference_on_these_rows(want, kind):
    from tests.emul import lmac_biterr_emul_bind, lmac_list_emul_bind, lmac_soft_emul_bind
    e = want[kind]
    for pre in ("", "list_"):
        rows, codes = e[pre + "rows"], None if kind == "sb1" else e[pre + "codes"]
        t2, ok = lmac_soft_emul_bind.decode_rows(kind, rows, codes)
        assert np.array_equal(t2, e[pre + "t2"]) and np.array_equal(ok, e[pre + "ok"]), (kind, pre)
        for T in (1, 4, 8):
            w_out, w_ok, w_rank = for_T(e[pre + "def"], T)
            out, ok, rank, be = lmac_list_emul_bind.decode_soft_rows(kind, rows, codes, T)
            assert np.array_equal(out, w_out) and np.array_equal(ok, w_ok) and np.array_equal(rank, w_rank), (kind, pre, T)
            assert np.array_equal(be, counts_after(e, pre, slice(None), w_out)), (kind, pre, T)
    t2, ok, be = lmac_biterr_emul_bind.decode_soft_rows(kind, e["rows"], None if kind == "sb1" else e["codes"])
    assert np.array_equal(t2, e["t2"]) and np.array_equal(ok, e["ok"]) and np.array_equal(be, e["biterr"]), kind


def test_extension_header_is_exported_and_bound(pkg):
    """tests/test_abi.py's rule for include/ext/tetra_soft.h: the function it declares is exported by the library, bound with the
    declared number of parameters in lmac_binding.SOFT_ABI (the ring size as 32 bits, every pointer pointer-wide), and the header
    compiles as C."""
    import re
    import subprocess
    hdr = os.path.join(ROOT, "include", "ext", "tetra_soft.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): [a.strip() for a in " ".join(m.group(2).split()).split(",")] for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    table = pkg.lmac_binding.SOFT_ABI
    assert list(decls) == ["tetra_lmac_decode_frames_soft_device"] == list(table) == pkg.lmac_binding.SOFT_EXPORTS
    L = pkg.load_library()
    pkg.lmac_binding._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        restype, argtypes = table[name]
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params) == 9
        for decl, ct in zip(params, argtypes):
            assert C.sizeof(ct) == (C.sizeof(C.c_void_p) if "*" in decl else 4), decl
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c++", hdr], check=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch, torch.device("cuda", 0)


class Plan:
    """The frames of a launch, on the host: frame f belongs to channel f // fpc; every channel's ring starts as junk of its own, and
    put() lays a row at a frame's burst positions.  Bit numbers unless given: channel c's frames 517 bits apart (every alignment) from
    6000 + 131 c on, so that with 8192 values a ring the last frames of a channel wrap its end."""

    def __init__(self, n_frames, fpc=FPC, ring_size=8192, seed=1, bitnum=None):
        self.n, self.fpc, self.ring_size = n_frames, fpc, ring_size
        self.channels = -(-n_frames // fpc)
        rng = np.random.default_rng(seed)
        self.rings = rng.integers(-31, 32, (self.channels, ring_size)).astype(np.int8)
        f = np.arange(n_frames)
        self.bitnum = (6000 + 131 * (f // fpc) + 517 * (f % fpc)).astype(np.uint32) if bitnum is None else np.array(bitnum, np.uint64).astype(np.uint32)
        self.types = np.full(n_frames, -1, np.int32)
        self.codes = rng.integers(0, 1 << 32, n_frames, dtype=np.uint64).astype(np.uint32)
        self.time_rx = rng.integers(0, 1 << 32, n_frames, dtype=np.uint64).astype(np.uint32)
        self.time = rng.integers(0, 1 << 32, n_frames, dtype=np.uint64).astype(np.uint32)
        self._dev = None

    def put(self, f, kind, row, code):
        _, _, train, pieces = sp.KINDS[kind]
        self.types[f], self.codes[f] = train, code
        at = 0
        for off, ln in pieces:
            idx = (int(self.bitnum[f]) + off + np.arange(ln)) % self.ring_size          # (the ring's size divides 2^32)
            self.rings[f // self.fpc, idx] = row[at:at + ln]
            at += ln
        assert at == len(row)

    def device(self, torch, dev):
        if self._dev is None:
            u32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
            self._dev = dict(frames=torch.zeros((self.n, 16), dtype=torch.int32, device=dev), types=torch.from_numpy(self.types).to(dev),
                             bitnum=u32(self.bitnum), codes=u32(self.codes), time_rx=u32(self.time_rx), time=u32(self.time),
                             ring=torch.from_numpy(self.rings).to(dev))
        return self._dev


def plan_of(items, **kw):
    """frame f carries items[f] = (kind, row, code)"""
    p = Plan(len(items), **kw)
    for f, (kind, row, code) in enumerate(items):
        p.put(f, kind, row, code)
    return p


def device_jobs(torch, dev, plan, jobs):
    """jobs: dicts with kind, listed (frames, int), and optionally max_rows (default: len(listed); rows past listed name frame 0), have (a
    device-side count), labels, biterr, rank (booleans) -> the binding's job dicts, every output poisoned."""
    d = plan.device(torch, dev)
    out = []
    for j in jobs:
        tpsap, blk, _, _ = sp.KINDS[j["kind"]]
        listed = np.asarray(j["listed"], np.int32)
        m = int(j.get("max_rows", len(listed)))
        lf = np.zeros(m, np.int32)
        lf[:min(m, len(listed))] = listed[:m]
        ost = sp.TYPE2_BITS[j["kind"]] + 8
        i32 = lambda fill, *shape: torch.full(shape, fill, dtype=torch.int32, device=dev)
        out.append(dict(type=tpsap, blk_num=blk, row_frame=torch.from_numpy(lf).to(dev), max_rows=m, out_stride=ost, frame_scramb=d["codes"],
                        n_rows=None if j.get("have") is None else torch.tensor([j["have"]], dtype=torch.int32, device=dev),
                        type2=torch.full((m, ost), 7, dtype=torch.uint8, device=dev), crc_ok=i32(-3, m),
                        labels=i32(-9, m, 6) if j.get("labels") else None, biterr=i32(SENTINEL, m) if j.get("biterr") else None,
                        rank=i32(SENTINEL, m) if j.get("rank") else None))
    return out


def launch(pkg, plan, jobs, T=4, stream=None, workspace=False, busy=None, counted=True, ranked=True):
    """One call of tetra_lmac_decode_frames_soft_device -> per job a dict of numpy arrays: type2 [max_rows][type2 + 8], ok, labels, biterr
    (uint32), rank (None where the job has none)."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    d = plan.device(torch, dev)
    dj = device_jobs(torch, dev, plan, jobs)
    ws = torch.zeros(max(4, lb.decode_frames_workspace_bytes(dj)), dtype=torch.uint8, device=dev) if workspace else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))            # the uploads and the poison
        for k in range(8 if busy is not None else 0):
            busy.fill_(k)                                             # the null stream is busy with something else meanwhile
    lb.decode_frames_soft(d["frames"], d["types"], dj, d["ring"], plan.ring_size, plan.fpc, d["bitnum"], max_candidates=T, d_time_rx=d["time_rx"],
                          d_time=d["time"], stream=stream, d_workspace=ws, counted=counted, ranked=ranked)
    torch.cuda.synchronize()
    host = lambda x, dt=None: None if x is None else (x.cpu().numpy() if dt is None else x.cpu().numpy().view(dt))
    return [dict(type2=host(j["type2"]), ok=host(j["crc_ok"]), labels=host(j["labels"]), biterr=host(j["biterr"], np.uint32), rank=host(j["rank"]))
            for j in dj]


def assert_rows(got, n2, want_t2, want_ok, what, upto=None):
    """rows [0, upto) are the expected bits and verdicts, the padding behind every row and every row from upto on are as poisoned"""
    upto = len(want_t2) if upto is None else upto
    assert np.array_equal(got["type2"][:upto, :n2], want_t2[:upto]) and np.array_equal(got["ok"][:upto], want_ok[:upto]), what
    assert (got["type2"][:, n2:] == 7).all(), what
    assert_untouched(got, upto, what)


def assert_untouched(got, upto, what):
    assert len(got["type2"]) >= upto and (got["type2"][upto:] == 7).all() and (got["ok"][upto:] == -3).all(), what
    for key, fill in (("labels", -9), ("biterr", SENTINEL), ("rank", SENTINEL)):
        if got[key] is not None:
            assert (got[key][upto:] == fill).all(), (what, key)


def assert_labels(got, plan, listed, what):
    lab = got["labels"][:len(listed)].view(np.uint32)
    f = np.asarray(listed)
    for col, exp in enumerate((f // plan.fpc, f % plan.fpc, plan.bitnum[f], plan.time_rx[f], plan.time[f], got["ok"][:len(f)])):
        assert np.array_equal(lab[:, col], np.asarray(exp).astype(np.uint32)), (what, col)


def batches(n, size=5 * FPC):
    return [np.arange(a, min(n, a + size)) for a in range(0, n, size)]


def decode_pool(pkg, e, kind, **job):
    """The planted rows of a kind, a frame each, 35 frames (5 channels of 7) a launch, one job per launch -> the launches' results joined"""
    parts = []
    for b, idx in enumerate(batches(len(e["rows"]))):
        plan = plan_of([(kind, e["rows"][i], e["codes"][i]) for i in idx], seed=10 + b)
        assert plan.channels == 5 and plan.fpc == 7 and plan.ring_size == 8192 and (np.diff(plan.bitnum[:7].astype(np.int64)) >= 510).all()
        n = len(idx)
        got = launch(pkg, plan, [dict(kind=kind, listed=np.arange(n), max_rows=n + 3, have=n, **job)])[0]
        assert_untouched(got, n, (kind, b))                              # the three rows past the count
        parts.append({k: None if v is None else v[:n] for k, v in got.items()})
    return {k: None if parts[0][k] is None else np.concatenate([p[k] for p in parts]) for k in parts[0]}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_planted_rows_of_every_kind_equal_the_reference(pkg, want, kind):
    """100 planted rows of the kind, each a frame, 5 channels of 7 frames with different junk in every channel's ring, the last frames
    of a channel across the ring's end: rows and verdicts are the reference's; the padding bytes behind every row and the rows past the
    device-side count are not touched."""
    e = want[kind]
    got = decode_pool(pkg, e, kind)
    assert_rows(got, sp.TYPE2_BITS[kind], e["t2"], e["ok"], kind)
    assert e["ok"].sum() >= 12 and got["type2"].shape == (100, sp.TYPE2_BITS[kind] + 8)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("schf", "sb1"))
def test_gpu_row_counts_at_the_workgroup_edge(pkg, want, kind):
    """max_rows / device-side count (1, 1) .. (130, 0) over a permuted frame list that names some frames twice, with labels, counts and
    ranks: rows below the count are the definition's, rows from the count on are untouched in every output."""
    e = want[kind]
    n2 = sp.TYPE2_BITS[kind]
    plan = plan_of([(kind, e["rows"][i], e["codes"][i]) for i in range(100)], seed=20)
    assert plan.channels == 15
    listed = np.resize(np.random.default_rng(21).permutation(100), 130)
    w_out, w_ok, w_rank = for_T(e["def"], 4)
    for max_rows, have in ((1, 1), (63, 63), (64, 64), (65, 65), (130, 65), (130, 0)):
        got = launch(pkg, plan, [dict(kind=kind, listed=listed, max_rows=max_rows, have=have, labels=True, biterr=True, rank=True)], T=4)[0]
        idx = listed[:have]
        assert_rows(got, n2, w_out[idx], w_ok[idx], (kind, max_rows, have), upto=have)
        assert np.array_equal(got["rank"][:have], w_rank[idx]) and np.array_equal(got["biterr"][:have], counts_after(e, "", idx, w_out[idx]))
        assert_labels(got, plan, idx, (kind, max_rows, have))
    assert len(set(listed[:65])) == 65 and len(set(listed)) < 130 and (w_rank[listed[:65]] > 0).any() and (w_rank[listed[:65]] == -1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("schf", "sb1"))
def test_gpu_ring_addressing(pkg, want, kind):
    """One noisy row at every alignment of its frame, across the ring's end at each piece, across the 2^32 wrap of the bit number, in
    the smallest ring that holds a burst and in a large one: the same answer every time, the reference's."""
    e = want[kind]
    row, code = e["rows"][1], e["codes"][1]
    first = sp.KINDS[kind][3][0][0]
    cases = {1024: list(range(8)) + [510, 1024 - 14 - 3, 1024 - 282 - 1, 1024 - first - 1, 1024 - first - 3, 0xffffffff, 0xfffffe03],
             512: [0, 5, 512 - first - 2, 0xffffffff, 0xfffffe03], 65536: [0, 3, 65536 - first - 1, 65536 - 300, 0xffffffff, 0xfffffe03]}
    for ring_size, bitnums in cases.items():
        plan = plan_of([(kind, row, code)] * len(bitnums), fpc=1, ring_size=ring_size, seed=30, bitnum=bitnums)      # a channel per case
        got = launch(pkg, plan, [dict(kind=kind, listed=np.arange(len(bitnums)), labels=True)])[0]
        n = len(bitnums)
        assert_rows(got, sp.TYPE2_BITS[kind], np.repeat(e["t2"][1:2], n, 0), np.repeat(e["ok"][1:2], n), (kind, ring_size))
        assert_labels(got, plan, np.arange(n), (kind, ring_size))
    assert e["t2"][1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_frames_of_other_burst_types_are_erasures(pkg, want, kind):
    """Frames of all three burst types listed under every layout: a frame that does not carry the kind decodes as the reference decodes
    an all-zero soft row under that frame's code, whatever its ring holds; a carrying frame between them decodes its row."""
    e = want[kind]
    train = sp.KINDS[kind][2]
    zero, rnd = np.arange(ZERO_ROWS.start, ZERO_ROWS.stop), np.arange(48, 52)
    plan = Plan(12, seed=40)
    src = []
    for f in range(12):
        ft, k = (0, 1, 3)[f % 3], f // 3
        if ft == train:
            plan.put(f, kind, e["rows"][rnd[k]], e["codes"][rnd[k]])
            src.append(rnd[k])
        else:
            plan.types[f], plan.codes[f] = ft, e["codes"][zero[k]]                # its ring positions stay junk
            src.append(zero[k])
    got = launch(pkg, plan, [dict(kind=kind, listed=np.arange(12), biterr=True)])[0]
    assert_rows(got, sp.TYPE2_BITS[kind], e["t2"][src], e["ok"][src], kind)
    assert np.array_equal(got["biterr"], e["biterr"][src]) and sorted(set(plan.types)) == [0, 1, 3] and e["t2"][rnd].any()


ORDER = ("schf", "sb2", "ndb1", "ndb2", "sb1")


def mixed_plan(want, seed):
    """35 frames, 5 channels: frame f carries a planted row of kind ORDER[f % 5] -> (plan, {kind: frames}, {kind: the rows' indices})"""
    items, frames, idx = [], {k: [] for k in ORDER}, {k: [] for k in ORDER}
    for f in range(5 * FPC):
        kind, i = ORDER[f % 5], (13 * f + 1) % 100
        items.append((kind, want[kind]["rows"][i], want[kind]["codes"][i]))
        frames[kind].append(f), idx[kind].append(i)
    return plan_of(items, seed=seed), frames, idx


@pytest.mark.gpu
def test_gpu_all_five_layouts_in_one_launch(pkg, want):
    """Jobs SCH/F, SB2, NDB 1, NDB 2, SB1 in one launch with labels: every label field, the label's verdict, rows and verdicts; with the
    caller's workspace and with the pool's; on a side stream while the null stream is busy."""
    torch, dev = _dev()
    plan, frames, idx = mixed_plan(want, 50)
    jobs = [dict(kind=k, listed=frames[k], labels=True) for k in ORDER]
    busy = torch.empty(1 << 27, dtype=torch.uint8, device=dev)
    for kw in (dict(workspace=True), dict(workspace=False), dict(workspace=False, stream=torch.cuda.Stream(dev), busy=busy),
               dict(workspace=True, stream=torch.cuda.Stream(dev), busy=busy)):
        for got, kind in zip(launch(pkg, plan, jobs, **kw), ORDER):
            e = want[kind]
            assert_rows(got, sp.TYPE2_BITS[kind], e["t2"][idx[kind]], e["ok"][idx[kind]], (kind, sorted(kw)))
            assert_labels(got, plan, frames[kind], (kind, sorted(kw)))
    assert sum(want[k]["ok"][idx[k]].sum() for k in ORDER) >= 5 and sum((want[k]["ok"][idx[k]] == 0).sum() for k in ORDER) >= 5


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_counting_instantiation(pkg, want, kind):
    """The planted rows with counts: the counts are the definition's on the reference's bits; rows and verdicts are those without."""
    e = want[kind]
    got = decode_pool(pkg, e, kind, biterr=True)
    assert_rows(got, sp.TYPE2_BITS[kind], e["t2"], e["ok"], kind)
    assert np.array_equal(got["biterr"], e["biterr"]), kind
    assert len(set(e["biterr"])) > 20


@pytest.mark.gpu
def test_gpu_counting_with_a_job_that_does_not_count(pkg, want):
    plan, frames, idx = mixed_plan(want, 60)
    got = launch(pkg, plan, [dict(kind=k, listed=frames[k], biterr=k != "ndb1") for k in ORDER])
    for g, kind in zip(got, ORDER):
        e = want[kind]
        assert_rows(g, sp.TYPE2_BITS[kind], e["t2"][idx[kind]], e["ok"][idx[kind]], kind)
        assert (g["biterr"] is None) == (kind == "ndb1")
        if kind != "ndb1":
            assert np.array_equal(g["biterr"], e["biterr"][idx[kind]]), kind
    # no count array at all: the plain instantiation
    for g, kind in zip(launch(pkg, plan, [dict(kind=k, listed=frames[k]) for k in ORDER], counted=False), ORDER):
        assert_rows(g, sp.TYPE2_BITS[kind], want[kind]["t2"][idx[kind]], want[kind]["ok"][idx[kind]], kind)


def list_plan(want, seed):
    """the 64 list rows of every kind, a frame each, kind after kind: 320 frames, 46 channels"""
    items = [(k, want[k]["list_rows"][i], want[k]["list_codes"][i]) for k in ORDER for i in range(64)]
    return plan_of(items, seed=seed), {k: np.arange(64) + 64 * n for n, k in enumerate(ORDER)}


@pytest.mark.gpu
def test_gpu_rescue_with_the_soft_front_end(pkg, want):
    """The list rows with ranks, T = 1, 4 and the documented maximum: rows, verdicts, label verdicts and ranks are the definition's; with
    counts as well a rescued row's count is that of the rescued codeword."""
    assert pkg.lmac_binding.LIST_MAX_CANDIDATES == 8
    plan, frames = list_plan(want, 70)
    for T, counts in ((1, False), (4, False), (8, False), (8, True), (4, True)):
        got = launch(pkg, plan, [dict(kind=k, listed=frames[k], labels=True, rank=True, biterr=counts) for k in ORDER], T=T)
        for g, kind in zip(got, ORDER):
            e = want[kind]
            w_out, w_ok, w_rank = for_T(e["list_def"], T)
            assert_rows(g, sp.TYPE2_BITS[kind], w_out, w_ok, (kind, T))
            assert np.array_equal(g["rank"], w_rank), (kind, T)
            assert_labels(g, plan, frames[kind], (kind, T))
            if counts:
                assert np.array_equal(g["biterr"], counts_after(e, "list_", slice(None), w_out)), (kind, T)
                ml = counts_after(e, "list_", slice(None), e["list_t2"])
                assert T != 8 or ((w_rank > 0) & (ml != g["biterr"])).any(), kind         # a count left at the ML row's would be noticed
            assert T == 1 or ((w_rank > 1).any() and (w_rank == -1).any()), (kind, T)


@pytest.mark.gpu
def test_gpu_rescue_leaves_good_rows_and_jobs_without_ranks_alone(pkg, want):
    plan, frames = list_plan(want, 80)
    # a launch with no failed row: every rank 0, every row the decoder's
    good = {k: frames[k][want[k]["list_ok"] == 1] for k in ORDER}
    for g, kind in zip(launch(pkg, plan, [dict(kind=k, listed=good[k], rank=True) for k in ORDER], T=8), ORDER):
        i = good[kind] - frames[kind][0]
        assert len(i) >= 10 and (g["rank"] == 0).all(), kind
        assert_rows(g, sp.TYPE2_BITS[kind], want[kind]["list_t2"][i], want[kind]["list_ok"][i], kind)
    # a mixed rank table: only the jobs with ranks are rescued
    ranked = ("schf", "ndb1", "sb1")
    for g, kind in zip(launch(pkg, plan, [dict(kind=k, listed=frames[k], rank=k in ranked) for k in ORDER], T=4), ORDER):
        e = want[kind]
        w_out, w_ok, w_rank = for_T(e["list_def"], 4)
        assert (w_rank > 0).any()
        if kind in ranked:
            assert_rows(g, sp.TYPE2_BITS[kind], w_out, w_ok, kind)
            assert np.array_equal(g["rank"], w_rank), kind
        else:
            assert g["rank"] is None
            assert_rows(g, sp.TYPE2_BITS[kind], e["list_t2"], e["list_ok"], kind)
    # no rank array at all: the decoder's rows
    for g, kind in zip(launch(pkg, plan, [dict(kind=k, listed=frames[k]) for k in ORDER], ranked=False), ORDER):
        assert_rows(g, sp.TYPE2_BITS[kind], want[kind]["list_t2"], want[kind]["list_ok"], kind)


@pytest.mark.gpu
def test_gpu_refusals_write_nothing(pkg, want):
    """TETRA_ERR_ARG with nothing written: no ring, a ring size of 0, 2 or 1000, a ring off the 4-byte grid, no bit numbers, no frames per
    channel, a BBK job with and without TETRA_LMAC_JOB_RM3014."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    plan, frames, idx = mixed_plan(want, 90)
    d = plan.device(torch, dev)
    fn = lb._lib().tetra_lmac_decode_frames_soft_device
    specs = [dict(kind=k, listed=frames[k], labels=True, biterr=True, rank=True) for k in ORDER]
    dj = device_jobs(torch, dev, plan, specs)
    bbk = dict(dj[1], type=lb.TPSAP_T_BBK, blk_num=0, biterr=None, rank=None)

    def call(jobs, ring=d["ring"].data_ptr(), ring_size=plan.ring_size, fpc=plan.fpc, bitnum=d["bitnum"]):
        src = lb._frames(d["frames"], d["types"], fpc, bitnum, d["time_rx"], d["time"], None)
        arr = lambda key: (C.c_void_p * len(jobs))(*[None if j.get(key) is None else j[key].data_ptr() for j in jobs])
        return fn(C.byref(src), lb._job_array(jobs), len(jobs), ring, ring_size, arr("biterr"), arr("rank"), 4, None)

    assert call(dj, ring=None) == ERR_ARG
    for size in (0, 2, 1000):
        assert call(dj, ring_size=size) == ERR_ARG, size
    for off in (1, 2, 3):
        assert call(dj, ring=d["ring"].data_ptr() + off) == ERR_ARG, off
    assert call(dj, bitnum=None) == ERR_ARG and call(dj, fpc=0) == ERR_ARG
    assert call(dj[:1] + [bbk] + dj[2:]) == ERR_ARG
    assert call(dj[:1] + [dict(bbk, type=lb.TPSAP_T_BBK | lb.JOB_RM3014)] + dj[2:]) == ERR_ARG
    torch.cuda.synchronize()
    for j in dj:
        assert (j["type2"] == 7).all() and (j["crc_ok"] == -3).all() and (j["labels"] == -9).all(), "a refused call wrote"
        assert (j["biterr"] == SENTINEL).all() and (j["rank"] == SENTINEL).all(), "a refused call wrote"
    # the same table is accepted as it stands
    assert call(dj) == 0
    torch.cuda.synchronize()
    for j, kind in zip(dj, ORDER):
        w_out, w_ok, _ = for_T({k: want[kind]["def"][k][idx[kind]] for k in ("rank", "out", "ml")}, 4)
        assert np.array_equal(j["type2"].cpu().numpy()[:, :sp.TYPE2_BITS[kind]], w_out) and np.array_equal(j["crc_ok"].cpu().numpy(), w_ok), kind
