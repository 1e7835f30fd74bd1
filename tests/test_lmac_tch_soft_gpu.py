"""TCH/4.8 and TCH/2.4 from soft values (include/ext/tetra_tch_soft.h) on the GPU: the int8 byte-row entry points (k_tch_rows_soft), the
soft frame decoder's TCH jobs from planted rings (k_tch_frames_soft) alone and beside the signalling kinds, and the refusals.  Expected
rows and counts are the reference's: from oracle/_ref where it is built (tests/tch_soft_definition.py chains its functions), else from
tests/golden/lmac_tch_soft_golden.npz, which tests/test_lmac_tch_soft.py holds against the reference whenever that is at hand.  Every
output is poisoned before a launch; everything is integer and every comparison exact."""
import ctypes as C

import numpy as np
import pytest

from tests import soft_pipeline as sp
from tests import tch_soft_definition as sd
from tests.test_lmac_soft_gpu import FPC, SENTINEL, Plan, assert_labels, device_jobs, plan_of

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_SIZE, ERR_ALIGN = -1, -6, -7          # include/tetra_demod.h
SCHF_PIECES = sp.KINDS["schf"][3]                  # both blocks of a normal downlink burst: ((offset, length), ...)
TRAIN_NORM_1 = sp.KINDS["schf"][2]


@pytest.fixture(scope="module")
def want():
    """Read-only: soft_<kind>, code_<kind>, want_<kind>, be_<kind> of tests/tch_soft_definition.py."""
    from oracle import ref_binding
    if ref_binding.available() and ref_binding.lmac_available():
        from tests.golden import make_lmac_tch_soft_golden as G
        z = G.make(ref_binding.lmac_lib())
        print("expected values from oracle/_ref")
    else:
        z = dict(sd.load_golden())
        print("expected values from tests/golden/lmac_tch_soft_golden.npz")
    for a in z.values():
        a.flags.writeable = False
    return z


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _u32(torch, a, dev):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).to(dev)          # (a copy: the pools are read-only)


def _of(want, kind):
    return want["soft_%d" % kind], want["code_%d" % kind], want["want_%d" % kind], want["be_%d" % kind]


# ---- byte rows ------------------------------------------------------------------------------------------------------------------------
def rows_call(pkg, kind, rows, table, index, n, have, stride, counts):
    """tetra_lmac_decode_tch_soft_counted_device on `rows` (int8 [m][432]) laid `stride` apart with junk between them -> (type2 rows with
    their padding, count words or None), outputs poisoned with 7 / SENTINEL"""
    torch, dev = _dev()
    n2 = sd.BLK[kind][1]
    ost = n2 + 8
    laid = np.full((len(rows), stride), 0x77, np.int8)
    laid[:, :432] = rows
    t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
    be = _u32(torch, np.full(n, SENTINEL), dev) if counts else None
    pkg.lmac_binding.decode_tch_soft_counted_device(kind, torch.from_numpy(laid).to(dev), n, None if have is None else torch.tensor([have], dtype=torch.int32, device=dev),
                                                    stride, _u32(torch, table, dev), None if index is None else torch.from_numpy(index.astype(np.int32)).to(dev), t2, ost, be)
    torch.cuda.synchronize()
    return t2.cpu().numpy(), None if be is None else be.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", sd.CODED)
def test_byte_rows_of_every_set_equal_the_reference(pkg, want, kind):
    """All 144 rows (three workgroups, the last one ragged), tight rows and rows 436 and 448 bytes apart, with and without counts."""
    rows, code, w, wbe = _of(want, kind)
    n2 = sd.BLK[kind][1]
    for stride in (432, 436, 448):
        for counts in (True, False):
            got, be = rows_call(pkg, kind, rows, code, None, len(rows), None, stride, counts)
            for name, _ in sd.SETS:
                s = sd.set_slice(name)
                assert np.array_equal(got[s, :n2], w[s]), (kind, stride, counts, name)
                assert be is None or np.array_equal(be[s], wbe[s]), (kind, stride, name)
            assert (got[:, n2:] == 7).all(), (kind, stride, counts)
    assert w.any() and len(set(wbe.tolist())) > 40


@pytest.mark.parametrize("kind", sd.CODED)
def test_byte_row_counts_at_the_workgroup_edge(pkg, want, kind):
    """Capacity / device-side count (1, 1) .. (130, 0) with an init index that names some codes twice: rows below the count are the
    reference's, rows from the count on and the padding behind every row are untouched."""
    rows, code, w, wbe = _of(want, kind)
    n2 = sd.BLK[kind][1]
    listed = np.resize(np.random.default_rng(31).permutation(100), 130)
    assert len(set(listed[:65])) == 65 and len(set(listed)) < 130
    for n, have in ((1, 1), (63, 63), (64, 64), (65, 65), (130, 65), (130, 0)):
        for counts in (True, False):
            got, be = rows_call(pkg, kind, rows[listed[:n]], code, listed[:n], n, have, 432, counts)
            assert np.array_equal(got[:have, :n2], w[listed[:have]]), (kind, n, have)
            assert (got[have:] == 7).all() and (got[:, n2:] == 7).all(), (kind, n, have)
            if counts:
                assert np.array_equal(be[:have], wbe[listed[:have]]) and (be[have:] == SENTINEL).all(), (kind, n, have)


@pytest.mark.parametrize("kind", sd.CODED)
def test_host_entry(pkg, want, kind):
    rows, code, w, wbe = _of(want, kind)
    lb = pkg.lmac_binding
    out, be = lb.decode_tch_soft(kind, rows[:70], code[:70], biterr=True)
    assert out.shape == (70, sd.BLK[kind][1]) and np.array_equal(out, w[:70]) and np.array_equal(be, wbe[:70])
    err, cmp_ = lb.split_biterr(be)
    assert (cmp_ <= 432).all() and (err <= cmp_).all()
    wide = np.full((70, 440), 0x11, np.int8)
    wide[:, :432] = rows[70:140]
    assert np.array_equal(lb.decode_tch_soft(kind, wide, code[70:140]), w[70:140])


# ---- frames from rings ----------------------------------------------------------------------------------------------------------------
def tch_jobs(torch, dev, plan, specs):
    """specs: dicts with kind (9 / 10), listed, and optionally max_rows, have, labels, biterr, rank -> the binding's job dicts, poisoned"""
    d = plan.device(torch, dev)
    out = []
    for j in specs:
        listed = np.asarray(j["listed"], np.int32)
        m = int(j.get("max_rows", len(listed)))
        lf = np.zeros(m, np.int32)
        lf[:min(m, len(listed))] = listed[:m]
        ost = (sd.BLK[j["kind"]][1] + 15) & ~7
        i32 = lambda fill, *shape: torch.full(shape, fill, dtype=torch.int32, device=dev)
        out.append(dict(type=j["kind"], blk_num=0, row_frame=torch.from_numpy(lf).to(dev), max_rows=m, out_stride=ost, frame_scramb=d["codes"],
                        n_rows=None if j.get("have") is None else torch.tensor([j["have"]], dtype=torch.int32, device=dev),
                        type2=torch.full((m, ost), 7, dtype=torch.uint8, device=dev), crc_ok=i32(-3, m),
                        labels=i32(-9, m, 6) if j.get("labels") else None, biterr=i32(SENTINEL, m) if j.get("biterr") else None,
                        rank=i32(SENTINEL, m) if j.get("rank") else None))
    return out


def run(pkg, plan, dj, entry="decode_frames_soft_tch", stream=None, workspace=False, busy=None, T=4):
    torch, dev = _dev()
    lb = pkg.lmac_binding
    d = plan.device(torch, dev)
    ws = torch.zeros(max(4, lb.decode_frames_workspace_bytes(dj)), dtype=torch.uint8, device=dev) if workspace else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream(dev))
        for k in range(8 if busy is not None else 0):
            busy.fill_(k)
    getattr(lb, entry)(d["frames"], d["types"], dj, d["ring"], plan.ring_size, plan.fpc, d["bitnum"], max_candidates=T, d_time_rx=d["time_rx"],
                       d_time=d["time"], stream=stream, d_workspace=ws)
    torch.cuda.synchronize()
    host = lambda x, dt=None: None if x is None else (x.cpu().numpy() if dt is None else x.cpu().numpy().view(dt))
    return [dict(type2=host(j["type2"]), ok=host(j["crc_ok"]), labels=host(j["labels"]), biterr=host(j["biterr"], np.uint32), rank=host(j["rank"])) for j in dj]


def assert_tch(got, n2, w, wbe, upto, what):
    """rows [0, upto) are the expected bits with verdict 1 (and the expected counts), everything else is as poisoned"""
    assert np.array_equal(got["type2"][:upto, :n2], w) and (got["ok"][:upto] == 1).all(), what
    assert (got["type2"][:, n2:] == 7).all() and (got["type2"][upto:] == 7).all() and (got["ok"][upto:] == -3).all(), what
    if got["biterr"] is not None:
        assert np.array_equal(got["biterr"][:upto], wbe) and (got["biterr"][upto:] == SENTINEL).all(), what
    if got["labels"] is not None:
        assert (got["labels"][upto:] == -9).all(), what


@pytest.mark.parametrize("kind", sd.CODED)
def test_frames_planted_rows_equal_the_reference(pkg, want, kind):
    """100 rows of every set, a frame each, 35 frames (5 channels of 7 with different junk in every ring, the last frames of a channel
    across the ring's end) a launch: rows, counts, verdicts of 1 and labels; three rows past the device-side count stay untouched."""
    torch, dev = _dev()
    rows, code, w, wbe = _of(want, kind)
    pick = sd.frames_pick()
    assert len(pick) == 100
    n2 = sd.BLK[kind][1]
    for b, a in enumerate(range(0, 100, 5 * FPC)):
        idx = pick[a:a + 5 * FPC]
        n = len(idx)
        plan = plan_of([("schf", rows[i], code[i]) for i in idx], seed=10 + b)
        assert plan.fpc == 7 and plan.ring_size == 8192 and (n < 35 or plan.channels == 5)
        for counts in (True, False):
            got = run(pkg, plan, tch_jobs(torch, dev, plan, [dict(kind=kind, listed=np.arange(n), max_rows=n + 3, have=n, labels=True, biterr=counts)]))[0]
            assert_tch(got, n2, w[idx], wbe[idx], n, (kind, b, counts))
            assert_labels(got, plan, np.arange(n), (kind, b))
            assert (got["biterr"] is None) == (not counts)


@pytest.mark.parametrize("kind", sd.CODED)
def test_frames_ring_addressing(pkg, want, kind):
    """One noisy row at every alignment of its frame, across the ring's end inside each of the two pieces, across the 2^32 wrap of the bit
    number, in the smallest ring that holds a burst and in a large one: the same answer every time, the reference's."""
    torch, dev = _dev()
    rows, code, w, wbe = _of(want, kind)
    i = sd.set_slice("gain").start + 1
    (o0, l0), (o1, l1) = SCHF_PIECES
    n2 = sd.BLK[kind][1]
    for ring_size in (512, 1024, 65536):
        bitnums = list(range(8)) + [ring_size - o0 - 1, ring_size - o0 - l0 + 3, ring_size - o1 - 2, ring_size - o1 - l1 + 1, 0xffffffff, 0xfffffe03,
                                    0xffffffff - o1 - 5]
        plan = plan_of([("schf", rows[i], code[i])] * len(bitnums), fpc=1, ring_size=ring_size, seed=30, bitnum=bitnums)      # a channel per case
        n = len(bitnums)
        got = run(pkg, plan, tch_jobs(torch, dev, plan, [dict(kind=kind, listed=np.arange(n), labels=True, biterr=True)]))[0]
        assert_tch(got, n2, np.repeat(w[i:i + 1], n, 0), np.repeat(wbe[i:i + 1], n), n, (kind, ring_size))
        assert_labels(got, plan, np.arange(n), (kind, ring_size))
    assert w[i].any() and wbe[i] & 0xffff


@pytest.mark.parametrize("kind", sd.CODED)
def test_frames_of_other_burst_types_are_erasures(pkg, want, kind):
    """Frames of all three burst types listed in a TCH job: a SYNC or NORM_2 frame decodes as the all-zero soft row under its own code, with
    a count of 0, whatever its ring holds; a NORM_1 frame between them decodes its row."""
    torch, dev = _dev()
    rows, code, w, wbe = _of(want, kind)
    zero = np.arange(sd.set_slice("zero").start, sd.set_slice("zero").stop)
    rnd = np.arange(sd.set_slice("random").start, sd.set_slice("random").start + 4)
    plan = Plan(12, seed=40)
    src = []
    for f in range(12):
        ft, k = (0, 1, 3)[f % 3], f // 3
        if ft == TRAIN_NORM_1:
            plan.put(f, "schf", rows[rnd[k]], code[rnd[k]])
            src.append(rnd[k])
        else:
            plan.types[f], plan.codes[f] = ft, code[zero[k]]                      # its ring positions stay junk
            src.append(zero[k])
    got = run(pkg, plan, tch_jobs(torch, dev, plan, [dict(kind=kind, listed=np.arange(12), biterr=True)]))[0]
    assert_tch(got, sd.BLK[kind][1], w[src], wbe[src], 12, kind)
    assert sorted(set(plan.types)) == [0, 1, 3] and w[rnd].any() and not wbe[zero].any()


# ---- beside the signalling kinds --------------------------------------------------------------------------------------------------------
SIGNALLING = ("schf", "sb1", "ndb1")


def mixed_plan(want, seed):
    """35 frames, 5 channels: frame f carries a planted row of SCH/F, SB1, NDB block 1, TCH/4.8 or TCH/2.4 by f % 5
    -> (plan, {kind: frames}, {kind: the rows' indices})"""
    from tests.golden import make_lmac_soft_golden as G
    order = SIGNALLING + sd.CODED
    items, frames, idx = [], {k: [] for k in order}, {k: [] for k in order}
    sig = {k: G.planted(k) for k in SIGNALLING}
    for f in range(5 * FPC):
        kind, i = order[f % 5], (13 * f + 1) % 100
        if kind in sd.CODED:
            items.append(("schf", want["soft_%d" % kind][sd.frames_pick()[i]], want["code_%d" % kind][sd.frames_pick()[i]]))
            idx[kind].append(sd.frames_pick()[i])
        else:
            items.append((kind, sig[kind][0][i], sig[kind][1][i]))
            idx[kind].append(i)
        frames[kind].append(f)
    return plan_of(items, seed=seed), frames, idx


def test_tch_jobs_beside_the_signalling_kinds(pkg, want):
    """SCH/F, SB1, NDB, TCH/4.8 and TCH/2.4 jobs in one call of tetra_lmac_decode_frames_soft_tch_device, with labels, counts, and ranks
    on the signalling jobs; with the caller's workspace and with the pool's, on the null stream and on a side stream while the null
    stream is busy.  The TCH rows and counts are the reference's; the signalling jobs' rows, verdicts, labels, counts and ranks are byte
    for byte those of the same call through tetra_lmac_decode_frames_soft_device without the TCH jobs."""
    torch, dev = _dev()
    plan, frames, idx = mixed_plan(want, 50)
    sig_specs = [dict(kind=k, listed=frames[k], labels=True, biterr=True, rank=True) for k in SIGNALLING]
    tch_specs = [dict(kind=k, listed=frames[k], labels=True, biterr=True) for k in sd.CODED]
    base = run(pkg, plan, device_jobs(torch, dev, plan, sig_specs), entry="decode_frames_soft")
    assert sum((b["rank"] > 0).sum() + (b["rank"] < 0).sum() for b in base) >= 1 and sum((b["ok"] == 1).sum() for b in base) >= 5
    busy = torch.empty(1 << 27, dtype=torch.uint8, device=dev)
    for kw in (dict(workspace=True), dict(workspace=False), dict(workspace=False, stream=torch.cuda.Stream(dev), busy=busy),
               dict(workspace=True, stream=torch.cuda.Stream(dev), busy=busy)):
        # the TCH jobs between the signalling jobs: the job order is the caller's
        dj = device_jobs(torch, dev, plan, sig_specs)
        tj = tch_jobs(torch, dev, plan, tch_specs)
        got = run(pkg, plan, [dj[0], tj[0], dj[1], tj[1], dj[2]], **kw)
        for g, b, kind in zip((got[0], got[2], got[4]), base, SIGNALLING):
            for key in ("type2", "ok", "labels", "biterr", "rank"):
                assert np.array_equal(g[key], b[key]), (kind, key, sorted(kw))
        for g, kind in zip((got[1], got[3]), sd.CODED):
            n = len(frames[kind])
            assert_tch(g, sd.BLK[kind][1], want["want_%d" % kind][idx[kind]], want["be_%d" % kind][idx[kind]], n, (kind, sorted(kw)))
            assert_labels(g, plan, frames[kind], (kind, sorted(kw)))
    # the signalling jobs alone through the new entry: what the existing entry gives
    for g, b in zip(run(pkg, plan, device_jobs(torch, dev, plan, sig_specs)), base):
        for key in ("type2", "ok", "labels", "biterr", "rank"):
            assert np.array_equal(g[key], b[key]), key


def test_refusals_write_nothing(pkg, want):
    """TETRA_ERR_ARG with nothing written for a TCH/7.2 job, a TCH job with a rank, no ring, a ring off the 4-byte grid, a ring size of 0, 2
    or 1000, no bit numbers, no frames per channel; TETRA_ERR_SIZE / _ALIGN for a TCH job's out_stride as for any job.  The existing soft
    entry refuses the table for its TCH jobs.  The table without the offending entry is then accepted."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    plan, frames, idx = mixed_plan(want, 90)
    d = plan.device(torch, dev)
    L = lb._lib()
    dj = device_jobs(torch, dev, plan, [dict(kind=k, listed=frames[k], labels=True, biterr=True, rank=True) for k in SIGNALLING])
    tj = tch_jobs(torch, dev, plan, [dict(kind=k, listed=frames[k], labels=True, biterr=True) for k in sd.CODED])
    table = [dj[0], tj[0], dj[1], tj[1], dj[2]]
    spare = torch.full((len(frames[9]),), SENTINEL, dtype=torch.int32, device=dev)

    def call(jobs, fn=L.tetra_lmac_decode_frames_soft_tch_device, ring=d["ring"].data_ptr(), ring_size=plan.ring_size, fpc=plan.fpc, bitnum=d["bitnum"]):
        src = lb._frames(d["frames"], d["types"], fpc, bitnum, d["time_rx"], d["time"], None)
        arr = lambda key: (C.c_void_p * len(jobs))(*[None if j.get(key) is None else j[key].data_ptr() for j in jobs])
        return fn(C.byref(src), lb._job_array(jobs), len(jobs), ring, ring_size, arr("biterr"), arr("rank"), 4, None)

    assert call(table[:1] + [dict(tj[0], type=lb.T_TCH_7_2, biterr=None)] + table[2:]) == ERR_ARG
    assert call(table[:1] + [dict(tj[0], rank=spare)] + table[2:]) == ERR_ARG
    assert call(table[:3] + [dict(tj[1], rank=spare)] + table[4:]) == ERR_ARG
    assert call(table, ring=None) == ERR_ARG
    for size in (0, 2, 1000):
        assert call(table, ring_size=size) == ERR_ARG, size
    for off in (1, 2, 3):
        assert call(table, ring=d["ring"].data_ptr() + off) == ERR_ARG, off
    assert call(table, bitnum=None) == ERR_ARG and call(table, fpc=0) == ERR_ARG
    assert call(table[:1] + [dict(tj[0], out_stride=288)] + table[2:]) == ERR_SIZE
    assert call(table[:1] + [dict(tj[0], out_stride=300)] + table[2:]) == ERR_ALIGN
    assert call(table, fn=L.tetra_lmac_decode_frames_soft_device) == ERR_ARG          # the existing entry: no TCH jobs
    assert call(tj, fn=L.tetra_lmac_decode_frames_soft_device) == ERR_ARG
    torch.cuda.synchronize()
    assert (spare == SENTINEL).all()
    for j in table:
        assert (j["type2"] == 7).all() and (j["crc_ok"] == -3).all() and (j["labels"] == -9).all() and (j["biterr"] == SENTINEL).all(), "a refused call wrote"
        assert j["rank"] is None or (j["rank"] == SENTINEL).all(), "a refused call wrote"
    # the same table is accepted as it stands
    assert call(table) == 0
    torch.cuda.synchronize()
    for j, kind in zip(tj, sd.CODED):
        n2 = sd.BLK[kind][1]
        assert np.array_equal(j["type2"].cpu().numpy()[:, :n2], want["want_%d" % kind][idx[kind]]) and (j["crc_ok"] == 1).all(), kind
        assert np.array_equal(j["biterr"].cpu().numpy().view(np.uint32), want["be_%d" % kind][idx[kind]]), kind
    for j in dj:
        assert not (j["crc_ok"] == -3).any() and not (j["rank"] == SENTINEL).any()
