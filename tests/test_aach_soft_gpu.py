"""The soft AACH decoder on the device (include/ext/tetra_aach_soft.h): the bare primitive, the frame decoder's soft BBK job and the
receive chain's TETRA_RX_FLAG_AACH_SOFT, against the numpy definition (tests/aach_soft_definition.py) and, for the chain, against the
reference-only host pipeline's fixture (tests/aach_soft_pipeline.py -> tests/golden/aach_soft_golden.npz).  Everything is integer: every
comparison is exact.  The rows are tests/test_aach_soft.py's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import aach_soft_definition as A
from tests import aach_soft_pipeline as P
from tests import list_definition as D
from tests import soft_pipeline as sp
from tests import test_aach_soft as T
from tests.chain_gpu import ragged_cuts, run_stream
from tests.golden import make_aach_soft_golden as GA
from tests.golden import make_lmac_soft_golden as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_TILE, WAVE_TILE = 128, 32                    # blocks per workgroup and per wavefront of k_aach_soft (tetra_lmac.hip)
ERR_ARG = -1

# The chain's stream (tests/aach_soft_pipeline.py: 5 downlinks, one second, Es/N0 = 9.5 dB, seed 9401), counted on the CPU by the host
# pipeline alone: AACH rows, those behind the first good SYNC PDU, and of those (equal to the sent codeword, accepted but wrong, refused)
# per decoder.  Maximum likelihood returns the four rows the radius-3 rule gives up on.
CHAIN_ROWS, CHAIN_ROWS_TIMED = 198, 181
CHAIN_SCORES = {"pass": (158, 23, 0), "rm": (177, 0, 4), "ml": (181, 0, 0)}


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


# ---- CPU: the fixture and the constants ----------------------------------------------------------------------------------------------
def test_fixture_scores_are_the_recorded_ones():
    g = GA.load()
    scores, timed, right, wrong = P.scores(g)
    assert (len(g["label"]), timed) == (CHAIN_ROWS, CHAIN_ROWS_TIMED) and scores == CHAIN_SCORES
    assert scores["ml"][0] > scores["rm"][0] > scores["pass"][0] and len(wrong) == 0 and right.min() >= 1
    assert os.path.getsize(GA.PATH) < 16384


def test_fixture_is_the_host_pipeline(synth):
    """tests/golden/aach_soft_golden.npz is what tests/golden/make_aach_soft_golden.py makes from oracle/_ref, and the quantiser it uses is
    the product's soft_pair (host build)."""
    from oracle import binding as ob, ref_binding
    if not (ref_binding.available() and ref_binding.lmac_available()):
        pytest.skip("oracle/_ref not built and the reference not present")
    again, g = GA.make(), np.load(GA.PATH)
    assert set(again) == set(g.files) and all(np.array_equal(again[k], g[k]) for k in again)
    from tests.emul import lmac_soft_emul_bind
    _, nb, sym, _ = ob.process_batch(P.stream_iq(synth)[:1], want_sym=True)
    z = sym[0][:nb[0] // 2]
    assert np.array_equal(lmac_soft_emul_bind.quantise(z)[0], sp.quantise_np(z))


# ---- GPU: the bare primitive ---------------------------------------------------------------------------------------------------------------
def primitive_pool():
    """the ties, the all-zero row, the extremes and the magnitude-1 rows first, then the 4000 random rows -> (rows, info, margin, dist)"""
    rows = np.concatenate([T.tie_rows(), T.special_rows(), T.random_rows()[0]])
    want = [np.concatenate([T.want(name)[i] for name in ("tie", "special", "random")]) for i in range(3)]
    return rows, want[0], want[1], want[2]


def run_primitive(pkg, rows, n, stride, outs=(True, True, True), extra=3):
    """n rows at the given stride with junk in every byte behind the 30 values; outputs poisoned, `extra` elements longer than n
    -> (words, dist, margin) as numpy, None where the pointer was NULL"""
    torch, dev = _dev()
    buf = np.random.default_rng(stride).integers(-128, 128, (max(n, 1), stride)).astype(np.int8)
    buf[:n, :30] = rows[:n, :30]
    d_in = torch.from_numpy(buf).to(dev)
    d_w = torch.full((n + extra,), 0x5a5a5a5a, dtype=torch.int32, device=dev) if outs[0] else None
    d_d = torch.full((n + extra,), 0x5a, dtype=torch.uint8, device=dev) if outs[1] else None
    d_m = torch.full((n + extra,), 0x5a5a, dtype=torch.int16, device=dev) if outs[2] else None
    pkg.lmac_binding.rm3014_soft_decode(d_in, n, stride, d_w, d_d, d_m)
    torch.cuda.synchronize()
    host = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)
    return host(d_w, np.uint32), host(d_d, np.uint8), host(d_m, np.uint16)


def assert_primitive(got, n, info, margin, dist, what):
    w, d, m = got
    if w is not None:
        assert np.array_equal(w[:n], A.codewords()[info[:n]]) and (w[n:] == 0x5a5a5a5a).all(), what
    if d is not None:
        assert np.array_equal(d[:n], dist[:n]) and (d[n:] == 0x5a).all(), what
    if m is not None:
        assert np.array_equal(m[:n], margin[:n]) and (m[n:] == 0x5a5a).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("stride", (32, 40))
def test_gpu_primitive_equals_numpy_at_every_row_count(pkg, stride):
    """n = 0, 1, around the wavefront's 32 and the workgroup's 128 blocks, 70, and all 4030 pooled rows (ties, the all-zero row, the
    extremes among the first 30): codeword, dist and margin are the definition's and nothing behind row n is written."""
    rows, info, margin, dist = primitive_pool()
    assert len(rows) == 4030 and (margin[:4] == 0).all() and info[4] == 0 and margin[4] == 0
    for n in (0, 1, WAVE_TILE - 1, WAVE_TILE, WAVE_TILE + 1, 70, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, len(rows)):
        assert_primitive(run_primitive(pkg, rows, n, stride), n, info, margin, dist, (stride, n))


@pytest.mark.gpu
def test_gpu_primitive_every_codeword_wins_once(pkg):
    info, margin, dist = T.want("every")
    got = run_primitive(pkg, T.every_codeword(), 16384, 32)
    assert_primitive(got, 16384, info, margin, dist, "every")
    assert np.array_equal(got[0][:16384], A.codewords()) and (got[1][:16384] == 0).all() and got[2][:16384].min() >= 8


@pytest.mark.gpu
def test_gpu_primitive_null_outputs_and_refusals(pkg):
    rows, info, margin, dist = primitive_pool()
    for outs in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        assert_primitive(run_primitive(pkg, rows, 70, 40, outs), 70, info, margin, dist, outs)
    torch, dev = _dev()
    fn = pkg.lmac_binding._lib().tetra_lmac_rm3014_soft_decode_device
    d_in = torch.zeros((4, 32), dtype=torch.int8, device=dev)
    d_w = torch.full((4,), 7, dtype=torch.int32, device=dev)
    assert fn(None, 0, 32, None, None, None, None) == 0 and fn(d_in.data_ptr(), -1, 32, d_w.data_ptr(), None, None, None) == ERR_ARG
    assert fn(None, 4, 32, d_w.data_ptr(), None, None, None) == ERR_ARG and fn(d_in.data_ptr(), 4, 28, d_w.data_ptr(), None, None, None) == ERR_ARG
    assert fn(d_in.data_ptr() + 1, 3, 32, d_w.data_ptr(), None, None, None) != 0 and fn(d_in.data_ptr(), 3, 34, d_w.data_ptr(), None, None, None) != 0
    torch.cuda.synchronize()
    assert (d_w.cpu().numpy() == 7).all()


# ---- GPU: the frame decoder's soft BBK job ------------------------------------------------------------------------------------------------
N_FRAMES, FPC = 70, 14                           # tests/test_aach_rm.py's shape: 5 channels x 14 frame slots
TYPES = (3, 0, 1, 0, 1, 3, 0)                    # TETRA_TRAIN_SYNC / NORM_1 / NORM_2 mixed
FOREIGN = {20: 2, 41: -1}                        # listed frames of no downlink burst type: 30 erasures
CODED = (("schf", 0), ("sb2", 3), ("ndb1", 1), ("ndb2", 1))          # the jobs beside the BBK job and the burst type that carries them


@functools.lru_cache(None)
def aach_plan():
    """70 frames: frame f is a burst of type TYPES[f % 7] (two are foreign) whose AACH positions hold pooled row f scrambled by sign
    under the frame's code, and whose coded blocks hold planted rows of tests/golden/make_lmac_soft_golden.py under the same code.
    The frames of a channel lie 517 bits apart in a ring of 8192 (every alignment; the last ones wrap its end), and frames 13 | 14 are
    the frames_per_channel edge.  -> (plan, the AACH's descrambled values int8 [70][32])"""
    from tests.test_lmac_soft_gpu import Plan
    rows = primitive_pool()[0]
    pick = np.concatenate([np.arange(30), 30 + 57 * np.arange(40)])           # the 30 chosen rows, then random ones
    plan = Plan(N_FRAMES, fpc=FPC, ring_size=8192, seed=77)
    values = np.zeros((N_FRAMES, 32), np.int8)
    for f in range(N_FRAMES):
        train = FOREIGN.get(f, TYPES[f % 7])
        code = int(plan.codes[f])
        for kind, carrier in CODED:
            if carrier == train:                                                # a clean planted codeword, moved from its own code to the frame's
                rows_k, codes_k = G.planted(kind)
                i = 4 * (f % 12)
                moved = D.scramb_seq(int(codes_k[i]), rows_k.shape[1]) ^ D.scramb_seq(code, rows_k.shape[1])
                plan.put(f, kind, A.descramble(rows_k[i], moved).astype(np.int8), code)
        plan.types[f] = train
        if f in FOREIGN:
            continue                                                            # its ring positions stay junk
        values[f] = rows[pick[f]]
        seq = D.scramb_seq(code, 30)
        at = 0
        for off, ln in T.PIECES[train]:
            idx = (int(plan.bitnum[f]) + off + np.arange(ln)) % plan.ring_size
            plan.rings[f // FPC, idx] = A.descramble(values[f, at:at + ln], seq[at:at + ln])
            at += ln
    return plan, values


def frame_jobs(pkg, plan, listed, bbk_type, max_rows=None, have=None, biterr=False, rank=False):
    """the binding's job dicts, outputs poisoned: SCH/F, SB2, NDB 1, NDB 2 over the frames that carry them, then (bbk_type not None)
    the BBK job over `listed`"""
    from tests.test_lmac_soft_gpu import device_jobs
    torch, dev = _dev()
    d = plan.device(torch, dev)
    jobs = device_jobs(torch, dev, plan, [dict(kind=k, listed=np.flatnonzero(plan.types == carrier), labels=True) for k, carrier in CODED])
    if bbk_type is not None:
        m = len(listed) if max_rows is None else max_rows
        lf = np.zeros(m, np.int32)
        lf[:min(m, len(listed))] = listed[:m]
        i32 = lambda fill, *shape: torch.full(shape, fill, dtype=torch.int32, device=dev)
        jobs.append(dict(type=bbk_type, blk_num=0, row_frame=torch.from_numpy(lf).to(dev), max_rows=m, out_stride=40, frame_scramb=d["codes"],
                         n_rows=None if have is None else torch.tensor([have], dtype=torch.int32, device=dev),
                         type2=torch.full((m, 40), 7, dtype=torch.uint8, device=dev), crc_ok=i32(-3, m), labels=i32(-9, m, 6),
                         biterr=i32(0x5a, m) if biterr else None, rank=i32(0x5a, m) if rank else None))
    return jobs


def launch_soft(pkg, plan, jobs):
    torch, dev = _dev()
    d = plan.device(torch, dev)
    pkg.lmac_binding.decode_frames_soft(d["frames"], d["types"], jobs, d["ring"], plan.ring_size, plan.fpc, d["bitnum"], d_time_rx=d["time_rx"],
                                        d_time=d["time"], counted=False, ranked=False)
    torch.cuda.synchronize()
    return [dict(type2=j["type2"].cpu().numpy(), ok=j["crc_ok"].cpu().numpy(), labels=j["labels"].cpu().numpy()) for j in jobs]


@pytest.mark.gpu
def test_gpu_soft_bbk_job_beside_the_other_kinds(pkg):
    """The soft BBK job beside SCH/F, SB2 and both NDB jobs in one call: BBK rows, verdicts and labels are the definition's at min_margin
    1 (absent), 25 and 930, with a device-side count below max_rows over a permuted list that names frames twice; the other kinds are
    byte for byte what the call gives without the BBK job."""
    from tests.test_lmac_soft_gpu import assert_labels
    lb = pkg.lmac_binding
    plan, values = aach_plan()
    assert sorted(set(plan.types)) == [-1, 0, 1, 2, 3] and plan.channels == 5 and not values[20].any() and not values[41].any()
    assert int(plan.bitnum[13]) + 510 > 8192 and plan.bitnum[14] < plan.bitnum[13]          # a wrapped frame, and the next channel's first
    alone = launch_soft(pkg, plan, frame_jobs(pkg, plan, None, None))
    listed = np.resize(np.random.default_rng(5).permutation(N_FRAMES), 100)
    for mm, flag in ((1, 0), (25, lb.job_aach_min_margin(25)), (930, lb.job_aach_min_margin(930)), (1, lb.job_aach_min_margin(1))):
        for max_rows, have in ((100, None), (100, 70), (ROW_TILE + 2, ROW_TILE + 1)):
            many = np.resize(listed, max_rows)
            got = launch_soft(pkg, plan, frame_jobs(pkg, plan, many, lb.TPSAP_T_BBK | lb.JOB_RM3014_SOFT | flag, max_rows=max_rows, have=have))
            for a, b in zip(alone, got[:4]):
                assert all(np.array_equal(a[k], b[k]) for k in a), (mm, max_rows)
            n = max_rows if have is None else have
            w_rows, w_ok = A.rows(values[many[:n]], mm)
            bbk = got[4]
            assert np.array_equal(bbk["type2"][:n, :32], w_rows) and np.array_equal(bbk["ok"][:n], w_ok), (mm, max_rows, have)
            assert (bbk["type2"][:, 32:] == 7).all() and (bbk["type2"][n:] == 7).all() and (bbk["ok"][n:] == -3).all() and (bbk["labels"][n:] == -9).all()
            assert_labels(bbk, plan, many[:n], (mm, max_rows, have))
    w_ok = {mm: A.rows(values, mm)[1] for mm in (1, 25, 930)}
    assert w_ok[1].sum() > w_ok[25].sum() > 0 == w_ok[930].sum() and (w_ok[1] == 0).sum() >= 7
    assert all(a["ok"][:len(np.flatnonzero(plan.types == c))].sum() > 0 for a, (_, c) in zip(alone, CODED))          # the other jobs decode something


@pytest.mark.gpu
def test_gpu_soft_bbk_job_refusals_write_nothing(pkg):
    """TETRA_ERR_ARG before anything is launched: the flag in tetra_lmac_decode_frames_device, on a type other than BBK, beside
    TETRA_LMAC_JOB_RM3014, with a d_biterr or a d_rank entry, with a min_margin above 930 or min_margin bits alone; a BBK job without
    the flag (with and without TETRA_LMAC_JOB_RM3014) in the soft entry point."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    plan, _ = aach_plan()
    d = plan.device(torch, dev)
    listed = np.arange(N_FRAMES)
    soft_fn, hard_fn = lb._lib().tetra_lmac_decode_frames_soft_device, lb._lib().tetra_lmac_decode_frames_device
    ML = lb.TPSAP_T_BBK | lb.JOB_RM3014_SOFT
    jobs = frame_jobs(pkg, plan, listed, ML, biterr=True, rank=True)

    def call(bbk_type, fn=soft_fn, with_biterr=False, with_rank=False):
        js = jobs[:4] + [dict(jobs[4], type=bbk_type)]
        src = lb._frames(d["frames"], d["types"], plan.fpc, d["bitnum"], d["time_rx"], d["time"], None)
        arr = lambda on, key: (C.c_void_p * len(js))(*[None] * 4 + [js[4][key].data_ptr() if on else None])
        if fn is hard_fn:
            return fn(C.byref(src), lb._job_array(js), len(js), None)
        return fn(C.byref(src), lb._job_array(js), len(js), d["ring"].data_ptr(), plan.ring_size, arr(with_biterr, "biterr"), arr(with_rank, "rank"), 4, None)

    assert call(ML, fn=hard_fn) == ERR_ARG
    assert call(lb.TPSAP_T_SB2 | lb.JOB_RM3014_SOFT) == ERR_ARG and call(lb.TPSAP_T_SCH_F | lb.JOB_RM3014_SOFT) == ERR_ARG
    assert call(ML | lb.JOB_RM3014) == ERR_ARG
    assert call(ML, with_biterr=True) == ERR_ARG and call(ML, with_rank=True) == ERR_ARG
    assert call(ML | (931 << 16)) == ERR_ARG and call(ML | (1023 << 16)) == ERR_ARG and call(lb.TPSAP_T_BBK | lb.job_aach_min_margin(25)) == ERR_ARG
    assert call(lb.TPSAP_T_BBK) == ERR_ARG and call(lb.TPSAP_T_BBK | lb.JOB_RM3014) == ERR_ARG
    torch.cuda.synchronize()
    for j in jobs:
        assert (j["type2"] == 7).all() and (j["crc_ok"] == -3).all() and (j["labels"] == -9).all(), "a refused call wrote"
    assert (jobs[4]["biterr"] == 0x5a).all() and (jobs[4]["rank"] == 0x5a).all()
    assert call(ML) == 0                                                     # the same table is accepted as it stands
    torch.cuda.synchronize()
    assert (jobs[4]["crc_ok"] >= 0).all()


# ---- GPU: the receive chain -------------------------------------------------------------------------------------------------------------
def expected_bbk(g, min_margin=1):
    """the fixture as tests/chain_gpu.py's collect gives a kind's rows"""
    rows, ok = A.rows(g["soft"], min_margin)
    return [(int(l[0]), int(l[1]), int(o), int(l[2]), int(l[3]), r[:30].tobytes()) for l, o, r in zip(g["label"], ok, rows)]


@pytest.fixture(scope="module")
def chain_iq(synth):
    return P.stream_iq(synth)


@pytest.mark.gpu
@pytest.mark.parametrize("one_stream", [False, True])
def test_gpu_chain_equals_the_host_pipeline_under_ragged_cuts(pkg, chain_iq, one_stream):
    """SOFT | AACH_SOFT: the BBK rows are the fixture's, row for row, however the stream is cut, on two streams and on one; every other
    kind is what the chain with SOFT alone gives."""
    R = pkg.rx_binding
    base = R.FLAG_SOFT | (R.FLAG_ONE_STREAM if one_stream else 0)
    cuts = ragged_cuts(P.SAMPLES)
    got = run_stream(pkg, chain_iq, cuts, flags=base | R.FLAG_AACH_SOFT)
    soft_only = run_stream(pkg, chain_iq, cuts, flags=base)
    key = lambda r: (r[0], r[1])
    assert sorted(got[R.KIND_BBK], key=key) == expected_bbk(GA.load())
    for k in range(R.N_KINDS):
        if k != R.KIND_BBK:
            assert got[k] == soft_only[k] and (k != R.KIND_SCH_F or len(got[k]) > 40), k
    assert [r[:2] + r[3:5] for r in got[R.KIND_BBK]] == [r[:2] + r[3:5] for r in soft_only[R.KIND_BBK]]
    assert all(r[2] == 1 for r in soft_only[R.KIND_BBK])


def one_call(pkg, iq, flags, min_margin=None):
    """the whole stream in one call -> the BBK fetch, rows_device's bytes 30 / 31, the two column fetches, the CRC-good delivery"""
    import torch
    R = pkg.rx_binding
    rx = pkg.RxChain(iq.shape[0], iq.shape[1], flags=flags)
    if min_margin is not None:
        rx.set_aach_min_margin(min_margin)
    rx.process(iq)
    rx.wait()
    blocks, t1 = rx.fetch(R.KIND_BBK)
    out = dict(blocks=blocks.copy(), t1=t1.copy(), dist=rx.fetch_aach_dist().copy(), margin=rx.fetch_aach_margin().copy(),
               stride=rx.rows_device(R.KIND_BBK)[1])
    dl = rx.deliver(kinds=1 << R.KIND_BBK, crc_good_only=True).wait()[R.KIND_BBK]
    out["good"] = (dl[0].copy(), dl[1].copy())
    ext = rx.deliver(kinds=1 << R.KIND_BBK, extras=R.EXT_ROW_AACH_DIST).wait()
    out["ext_dist"] = np.array(ext.columns[R.KIND_BBK]["aach_dist"])
    rx.close()
    return out


@pytest.mark.gpu
def test_gpu_chain_columns_delivery_and_min_margin(pkg, chain_iq):
    """fetch_aach_dist, fetch_aach_margin and the CRC-good delivery agree with the rows; set_aach_min_margin(25) changes verdicts only."""
    R = pkg.rx_binding
    g = GA.load()
    flags = R.FLAG_SOFT | R.FLAG_AACH_SOFT
    runs = {mm: one_call(pkg, chain_iq, flags, mm) for mm in (None, 25)}
    for mm, run in runs.items():
        w_rows, w_ok = A.rows(g["soft"], 1 if mm is None else mm)
        b = run["blocks"]
        assert len(b) == CHAIN_ROWS and run["stride"] == 32
        assert np.array_equal(run["t1"], w_rows[:, :30]) and np.array_equal(b["crc_ok"], w_ok), mm
        assert np.array_equal(np.stack([b["channel"], b["bitnum"], b["tdma_time_rx"], b["tdma_time"]], axis=1).astype(np.int64), g["label"])
        assert np.array_equal(run["dist"], w_rows[:, 30]) and np.array_equal(run["margin"], w_rows[:, 31].astype(np.uint16)), mm
        assert run["dist"].dtype == np.uint8 and run["margin"].dtype == np.uint16
        keep = w_ok != 0
        gb, gt = run["good"]
        assert np.array_equal(gb, b[keep]) and np.array_equal(gt[:, :30], run["t1"][keep]), mm
        assert np.array_equal(run["ext_dist"], run["dist"]), mm                # the extended delivery's AACH_DIST column
    a, b = runs[None], runs[25]
    assert np.array_equal(a["t1"], b["t1"]) and np.array_equal(a["dist"], b["dist"]) and np.array_equal(a["margin"], b["margin"])
    assert b["blocks"]["crc_ok"].sum() < a["blocks"]["crc_ok"].sum() and len(b["good"][0]) < len(a["good"][0])
    info, _, _ = A.decode(g["soft"])
    post = (g["label"][:, 3] >> 16) != 0
    sent = P.sent_info()[g["label"][post, 0], P.slots_of(g["label"])[post]]
    assert int((info[post] == sent).sum()) == CHAIN_SCORES["ml"][0] > CHAIN_SCORES["rm"][0]


@pytest.mark.gpu
def test_gpu_create_and_setter_rules_and_the_upper_layers(pkg):
    R = pkg.rx_binding
    for flags in (R.FLAG_AACH_SOFT, R.FLAG_AACH_SOFT | R.FLAG_ONE_STREAM, R.FLAG_SOFT | R.FLAG_AACH_SOFT | R.FLAG_AACH_RM3014,
                  R.FLAG_AACH_SOFT | R.FLAG_AACH_RM3014, R.FLAG_SOFT | R.FLAG_AACH_SOFT | 4, R.FLAG_SOFT | 2048):
        with pytest.raises(pkg.TetraDemodError) as e:
            pkg.RxChain(2, 2000, flags=flags)
        assert e.value.status == ERR_ARG, flags
    for extra in (0, R.FLAG_ONE_STREAM, R.FLAG_BITERR, R.FLAG_LIST, R.FLAG_SYNC_TOLERANT, R.FLAG_BITERR | R.FLAG_LIST | R.FLAG_SYNC_TOLERANT):
        rx = pkg.RxChain(2, 2000, flags=R.FLAG_SOFT | R.FLAG_AACH_SOFT | extra)
        assert rx.fetch_aach_margin().size == 0 and rx.fetch_aach_dist().size == 0 and rx.fetch_aach_margin(1).size == 0
        for bad in (0, -1, 931, 1 << 16):
            with pytest.raises(pkg.TetraDemodError) as e:
                rx.set_aach_min_margin(bad)
            assert e.value.status == ERR_ARG
        rx.set_aach_min_margin(1), rx.set_aach_min_margin(930)
        rx.close()
    rx = pkg.RxChain(2, 2000, flags=R.FLAG_SOFT)
    for fn in (lambda: rx.set_aach_min_margin(5), rx.fetch_aach_margin, rx.fetch_aach_dist):
        with pytest.raises(pkg.TetraDemodError):
            fn()
    rx.close()
    rx = pkg.RxChain(2, 2000, flags=R.FLAG_SOFT | R.FLAG_AACH_SOFT, kinds=1 << R.KIND_SCH_F)          # a handle that does not decode BBK
    with pytest.raises(pkg.TetraDemodError):
        rx.fetch_aach_margin()
    rx.close()
    wb = pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=1 << 16, flags=R.FLAG_SOFT | R.FLAG_AACH_SOFT)
    assert wb.fetch_aach_margin().size == 0 and wb.rx.fetch_aach_dist().size == 0
    wb.set_aach_min_margin(25)
    with pytest.raises(pkg.TetraDemodError):
        wb.set_aach_min_margin(0)
    wb.close()
    with pytest.raises(pkg.TetraDemodError):
        pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=1 << 16, flags=R.FLAG_AACH_SOFT)


@pytest.mark.gpu
def test_gpu_host_banks_pass_the_flag_the_setter_and_the_margins(pkg, chain_iq, tmp_path):
    """TetraRxBank::setAachMinMargin / fetchAachMargin and the TetraRxMultiBank pass-through (host/tetra_rx_bank.h), 3 shards on one GPU
    against one bank of all channels and a soft-only bank: a plain C++ driver (tests/host/test_aach_soft_bank.cpp)."""
    pk = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd")
    pkg.build.build()
    exe = os.path.join(ROOT, "tests", "host", "test_aach_soft_bank")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pk, "host"),
                    os.path.join(ROOT, "tests", "host", "test_aach_soft_bank.cpp"), "-L", pk, "-ltetra_demod_hip", "-Wl,-rpath," + pk, "-o", exe], check=True)
    calls, N = 2, 9000
    f = tmp_path / "iq.bin"
    with open(f, "wb") as fh:
        for k in range(calls):
            fh.write(np.ascontiguousarray(chain_iq[:, k * N:(k + 1) * N]).astype(np.complex64).tobytes())
    r = subprocess.run([exe, str(P.CHANNELS), str(N), str(calls), str(f), "3", "25"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "test_aach_soft_bank: ok" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    assert int(r.stdout.split()[3]) > 40 and int(r.stdout.split()[5]) >= 1
