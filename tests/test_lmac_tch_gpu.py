"""Circuit-mode data channels TCH/7.2, TCH/4.8, TCH/2.4 (include/ext/tetra_tch.h) on the GPU: the byte-row entry points, the frame
decoder's TCH jobs beside the signalling kinds, and the statuses.  The expected rows and bit-error words are the reference's
(tests/golden/lmac_tch_golden.npz, which tests/test_lmac_tch.py holds against the reference's functions where they are built)."""
import numpy as np
import pytest

from tests import soft_pipeline as sp
from tests import tch_definition as td

pytestmark = pytest.mark.gpu
SENTINEL = 0x5a5a5a5a
ERR_ARG, ERR_SIZE, ERR_ALIGN = -1, -6, -7          # include/tetra_demod.h
KINDS = (td.TCH_7_2,) + td.CODED
SCHF_PIECES = sp.KINDS["schf"][3]                  # both blocks of a normal downlink burst: ((offset, length), ...)


@pytest.fixture(scope="module")
def golden():
    return td.load_golden()


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _u32(torch, a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)


def _pool(golden, kind, plain):
    """130 rows of a kind with their codes, expected rows and bit-error words: plain 0 / 1 rows (the packed route can take them), or rows
    that begin and end with arbitrary bytes."""
    names = [n for n, _, _ in td.sets_of(golden, kind)]
    order = [n for n in (("noisy", "bits") if plain else ("bytes",)) if n in names]
    sets = {n: (r, c) for n, r, c in td.sets_of(golden, kind)}
    rows = np.concatenate([sets[n][0] for n in order])[:130]
    code = np.concatenate([sets[n][1] for n in order])[:130]
    want = np.concatenate([golden["want_%d_%s" % (kind, n)] for n in order])[:130]
    be = np.concatenate([golden["be_%d_%s" % (kind, n)] for n in order])[:130] if kind in td.CODED else None
    assert len(rows) == 130
    return rows, code, want, be


@pytest.mark.parametrize("kind", KINDS)
def test_byte_rows_equal_the_reference(pkg, golden, kind):
    """tetra_lmac_decode_tch_counted_device at the 64-row workgroup edge (1, 63, 64, 65, 130 rows), the packed route and the byte route
    forced, plain rows and arbitrary bytes, tight rows and an in_stride (436) that forces the byte route: every row and every bit-error
    word is the reference's, with and without a count array."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    n2 = td.BLK[kind][1]
    ost = (n2 + 3) & ~3
    for plain in (True, False):
        rows_all, code_all, want_all, be_all = _pool(golden, kind, plain)
        for n in (1, 63, 64, 65, 130):
            for stride in (432, 436):
                rows = np.full((n, stride), 0x33, np.uint8)
                rows[:, :432] = rows_all[:n]
                d_rows, d_si = torch.from_numpy(rows).to(dev), _u32(torch, code_all[:n], dev)
                for forced in (False, True):
                    t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
                    t2p = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
                    be = _u32(torch, np.full(n, SENTINEL), dev) if kind in td.CODED else None
                    lb.force_byte_route(forced)
                    try:
                        lb.decode_tch_counted_device(kind, d_rows, n, None, stride, d_si, None, t2, ost, be)
                        lb.decode_tch_counted_device(kind, d_rows, n, None, stride, d_si, None, t2p, ost, None)
                        torch.cuda.synchronize()
                    finally:
                        lb.force_byte_route(False)
                    where = (kind, plain, n, stride, forced)
                    assert torch.equal(t2, t2p), where
                    assert np.array_equal(t2.cpu().numpy()[:, :n2], want_all[:n]), where
                    if be is not None:
                        assert np.array_equal(be.cpu().numpy().view(np.uint32), be_all[:n]), where


@pytest.mark.parametrize("kind", KINDS)
def test_counted_form_leaves_the_rows_past_the_count(pkg, golden, kind):
    """*d_n_blocks below the capacity: rows and count words past it keep their sentinel; the codes go through d_init_index."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    rows, code, want, be_want = _pool(golden, kind, True)
    n, have, n2 = 130, 70, td.BLK[kind][1]
    ost = (n2 + 3) & ~3
    perm = np.random.default_rng(5).permutation(n).astype(np.int32)
    table = np.zeros(n, np.uint32)
    table[perm] = code                          # row j's code sits at table[perm[j]]
    t2 = torch.full((n, ost), 7, dtype=torch.uint8, device=dev)
    be = _u32(torch, np.full(n, SENTINEL), dev) if kind in td.CODED else None
    lb.decode_tch_counted_device(kind, torch.from_numpy(np.ascontiguousarray(rows)).to(dev), n, torch.tensor([have], dtype=torch.int32, device=dev), 432,
                                 _u32(torch, table, dev), torch.from_numpy(perm).to(dev), t2, ost, be)
    torch.cuda.synchronize()
    got = t2.cpu().numpy()
    assert (got[have:] == 7).all() and np.array_equal(got[:have, :n2], want[:have])
    if be is not None:
        w = be.cpu().numpy().view(np.uint32)
        assert (w[have:] == SENTINEL).all() and np.array_equal(w[:have], be_want[:have])
    # n_blocks == 0 is a no-op
    lb.decode_tch_counted_device(kind, None, 0, None, 432, None, None, None, ost, None)


@pytest.mark.parametrize("kind", KINDS)
def test_host_entry(pkg, golden, kind):
    rows, code, want, be_want = _pool(golden, kind, False)
    lb = pkg.lmac_binding
    if kind in td.CODED:
        out, be = lb.decode_tch(kind, rows[:70], code[:70], biterr=True)
        assert np.array_equal(be, be_want[:70])
        err, cmp_ = lb.split_biterr(be)
        assert (cmp_ <= 432).all() and (err <= cmp_).all()
    else:
        out = lb.decode_tch(kind, rows[:70], code[:70])
    assert out.shape == (70, td.BLK[kind][1]) and np.array_equal(out, want[:70])


def _pack(burst_bits):
    b = np.zeros(512, np.uint8)
    b[:len(burst_bits)] = burst_bits
    return np.packbits(b).view(">u4").astype(np.uint32)


def _cut(burst_bits):
    return np.concatenate([burst_bits[o:o + n] for o, n in SCHF_PIECES])


def test_frames_tch_job_beside_the_signalling_kinds(pkg, golden):
    """Three channels x five planted packed frames of mixed types.  One call holds an SCH/F job, a BBK job and a TCH/4.8 job (with
    counts) over the same list -- the NORM_1 frames and one SYNC frame: the TCH rows and counts equal the two-step route (byte rows
    through the batch entry), its verdicts are 1 and its labels the frames'; the SCH/F and BBK rows, verdicts and labels are byte for byte
    those of the same call without the TCH job; the listed SYNC frame decodes as the all-zero block.  Then TCH/2.4 and TCH/7.2 jobs in a
    call of their own, and the workspace size."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    rng = np.random.default_rng(77)
    C_, F = 3, 5
    types = np.array([3, 0, 1, 0, 0] * C_, np.int32)            # SYNC, NORM_1, NORM_2, NORM_1, NORM_1 per channel
    bursts = rng.integers(0, 2, (C_ * F, 510)).astype(np.uint8)
    codes = td.codes(rng, C_ * F)
    norm1 = [f for f in range(C_ * F) if types[f] == 0]
    for k, f in enumerate(norm1):                               # TCH/4.8 blocks with a few errors in the NORM_1 frames' two blocks
        blk = golden["noisy_9"][k]
        codes[f] = golden["code_9"][k]
        at = 0
        for o, n in SCHF_PIECES:
            bursts[f, o:o + n] = blk[at:at + n]
            at += n
    packed = np.stack([_pack(b) for b in bursts])
    listed = np.array(norm1 + [5], np.int32)                    # ... and channel 1's SYNC frame
    n = len(listed)
    d_fr, d_ft, d_codes = _u32(torch, packed, dev), torch.from_numpy(types).to(dev), _u32(torch, codes, dev)
    bitnum = torch.arange(C_ * F, dtype=torch.int32, device=dev) * 510 + 7
    t_rx = torch.arange(C_ * F, dtype=torch.int32, device=dev) + 1000
    t_af = torch.arange(C_ * F, dtype=torch.int32, device=dev) + 5000
    d_list = torch.from_numpy(np.concatenate([listed, np.zeros(3, np.int32)])).to(dev)
    cap = n + 3

    def job(kind, width, counts=False):
        j = dict(type=kind, blk_num=0, row_frame=d_list, n_rows=torch.tensor([n], dtype=torch.int32, device=dev), max_rows=cap, out_stride=width,
                 frame_scramb=d_codes, type2=torch.full((cap, width), 5, dtype=torch.uint8, device=dev),
                 crc_ok=torch.full((cap,), -3, dtype=torch.int32, device=dev), labels=torch.full((cap, 6), -1, dtype=torch.int32, device=dev))
        if counts:
            j["biterr"] = _u32(torch, np.full(cap, SENTINEL), dev)
        return j
    mixed = [job(5, 296), job(3, 32), job(lb.T_TCH_4_8, 296, counts=True)]
    plain = [job(5, 296), job(3, 32)]
    lb.decode_frames_biterr_device(d_fr, d_ft, mixed, F, bitnum, t_rx, t_af)
    lb.decode_frames_device(d_fr, d_ft, plain, F, bitnum, t_rx, t_af)
    torch.cuda.synchronize()
    for m, p in zip(mixed, plain):
        for k in ("type2", "crc_ok", "labels"):
            assert torch.equal(m[k], p[k]), (m["type"], k)
    # the two-step route
    rows = np.stack([_cut(bursts[f]) if types[f] == 0 else np.zeros(432, np.uint8) for f in listed])
    want, want_be = lb.decode_tch(lb.T_TCH_4_8, rows, codes[listed], biterr=True)
    t = mixed[2]
    got = t["type2"].cpu().numpy()
    assert np.array_equal(got[:n, :292], want) and (got[n:] == 5).all()
    assert np.array_equal(want[:len(norm1)], golden["want_9_noisy"][:len(norm1)])
    zero, zero_be = lb.decode_tch(lb.T_TCH_4_8, np.zeros((1, 432), np.uint8), codes[5:6], biterr=True)
    assert np.array_equal(got[n - 1, :292], zero[0])                            # the SYNC frame: the all-zero block's result
    be = t["biterr"].cpu().numpy().view(np.uint32)
    assert np.array_equal(be[:n], want_be) and (be[n:] == SENTINEL).all() and be[n - 1] == zero_be[0]
    assert np.array_equal(be[:len(norm1)], golden["be_9_noisy"][:len(norm1)])
    ok = t["crc_ok"].cpu().numpy()
    assert (ok[:n] == 1).all() and (ok[n:] == -3).all()
    lab = t["labels"].cpu().numpy()
    assert np.array_equal(lab[:n], plain[0]["labels"].cpu().numpy()[:n] | np.array([0, 0, 0, 0, 0, 1])) and (lab[n:] == -1).all()
    assert np.array_equal(lab[:n, 0], listed // F) and np.array_equal(lab[:n, 1], listed % F) and np.array_equal(lab[:n, 2], listed * 510 + 7)
    # TCH jobs alone: TCH/2.4 (its own blocks planted), TCH/7.2, TCH/4.8 without counts, through the plain entry point and a workspace
    bursts2 = bursts.copy()
    codes2 = codes.copy()
    for k, f in enumerate(norm1):
        blk = golden["noisy_10"][k]
        codes2[f] = golden["code_10"][k]
        at = 0
        for o, ln in SCHF_PIECES:
            bursts2[f, o:o + ln] = blk[at:at + ln]
            at += ln
    d_fr2, d_codes2 = _u32(torch, np.stack([_pack(b) for b in bursts2]), dev), _u32(torch, codes2, dev)
    alone = [dict(job(lb.T_TCH_2_4, 152), frame_scramb=d_codes2), dict(job(lb.T_TCH_7_2, 432), frame_scramb=d_codes2),
             dict(job(lb.T_TCH_4_8, 296), frame_scramb=d_codes2)]
    need = lb.decode_frames_workspace_bytes(alone)
    groups = (cap + 63) // 64
    assert need == groups * 64 * 4 * ((148 + 4) // 2 + (292 + 4) // 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    lb.decode_frames_device(d_fr2, d_ft, alone, F, bitnum, t_rx, t_af, d_workspace=ws)
    torch.cuda.synchronize()
    rows2 = np.stack([_cut(bursts2[f]) if types[f] == 0 else np.zeros(432, np.uint8) for f in listed])
    for j, kind in zip(alone, (lb.T_TCH_2_4, lb.T_TCH_7_2, lb.T_TCH_4_8)):
        n2 = td.BLK[kind][1]
        got = j["type2"].cpu().numpy()
        assert np.array_equal(got[:n, :n2], lb.decode_tch(kind, rows2, codes2[listed])), kind
        assert (got[n:] == 5).all() and (j["crc_ok"].cpu().numpy()[:n] == 1).all()
    assert np.array_equal(alone[0]["type2"].cpu().numpy()[:len(norm1), :148], golden["want_10_noisy"][:len(norm1)])


def test_statuses(pkg):
    """TETRA_ERR_ARG for counts with TCH/7.2, for a TCH job on the soft and the list entry points and for a kind the entry point does not
    know; TETRA_ERR_ALIGN / _ARG / _SIZE for rows as documented; the one-kind entry points of tetra_lmac.h refuse 8..10 as before."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    L = pkg.binding.load_library()
    lb._lib()
    rows = torch.zeros((4, 440), dtype=torch.uint8, device=dev)
    si = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.zeros((4, 432), dtype=torch.uint8, device=dev)
    okd = torch.zeros(4, dtype=torch.int32, device=dev)
    bed = torch.zeros(8, dtype=torch.int32, device=dev)
    f = L.tetra_lmac_decode_tch_counted_device
    r, s, o, b = rows.data_ptr(), si.data_ptr(), out.data_ptr(), bed.data_ptr()
    assert f(8, r, 4, None, 440, s, None, o, 432, b, None) == ERR_ARG           # TCH/7.2 is not coded
    assert f(8, r, 4, None, 440, s, None, o, 432, None, None) == 0
    assert f(9, r, 4, None, 440, s, None, o, 292, b, None) == 0
    assert f(9, r, 4, None, 440, s, None, o, 292, b + 2, None) == ERR_ALIGN
    assert f(9, r + 2, 4, None, 440, s, None, o, 292, None, None) == ERR_ALIGN   # rows that are not 4-byte aligned
    assert f(9, r, 4, None, 438, s, None, o, 292, None, None) == ERR_ALIGN
    assert f(9, r, 4, None, 440, s, None, o + 1, 292, None, None) == ERR_ALIGN
    assert f(9, r, 4, None, 440, s, None, o, 294, None, None) == ERR_ALIGN
    assert f(9, r, 4, None, 428, s, None, o, 292, None, None) == ERR_ARG         # rows shorter than the block
    assert f(9, r, 4, None, 440, s, None, o, 288, None, None) == ERR_ARG
    assert f(10, r, 4, None, 440, None, None, o, 148, None, None) == ERR_ARG
    assert f(9, r, -1, None, 440, s, None, o, 292, None, None) == ERR_ARG
    for kind in (5, 7, 11, 9 | 0x100):
        assert f(kind, r, 4, None, 440, s, None, o, 432, None, None) == ERR_ARG
    # tetra_lmac.h's one-kind entry points: what they always returned
    for kind in (8, 9, 10):
        assert L.tetra_lmac_decode_counted_device(kind, r, 4, None, 440, s, None, o, 432, okd.data_ptr(), None) == ERR_ARG
        assert L.tetra_lmac_decode_batch_device(kind, r, 4, 440, s, o, 432, okd.data_ptr(), None) == ERR_ARG
        assert L.tetra_lmac_decode_counted_biterr_device(kind, r, 4, None, 440, s, None, o, 432, okd.data_ptr(), b, None) == ERR_ARG
        assert L.tetra_lmac_decode_counted_list_device(kind, r, 4, None, 440, s, None, o, 432, okd.data_ptr(), 4, b, None) == ERR_ARG
    # frame jobs
    frames = torch.zeros((4, 16), dtype=torch.int32, device=dev)
    ftype = torch.zeros(4, dtype=torch.int32, device=dev)
    bitnum = torch.arange(4, dtype=torch.int32, device=dev) * 510
    lst = torch.arange(4, dtype=torch.int32, device=dev)

    def job(kind, width, **kw):
        return dict(dict(type=kind, blk_num=0, row_frame=lst, n_rows=None, max_rows=4, out_stride=width, frame_scramb=si,
                         type2=torch.zeros((4, 432), dtype=torch.uint8, device=dev), crc_ok=okd, labels=None), **kw)

    def status(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except pkg.TetraDemodError as e:
            return e.status
        return 0
    ring = torch.zeros((1, 1024), dtype=torch.int8, device=dev)
    assert status(lb.decode_frames_device, frames, ftype, [job(9, 296)]) == 0
    assert status(lb.decode_frames_soft, frames, ftype, [job(9, 296)], ring, 1024, 4, bitnum) == ERR_ARG
    assert status(lb.decode_frames_soft, frames, ftype, [job(5, 288)], ring, 1024, 4, bitnum) == 0
    assert status(lb.decode_frames_list_device, frames, ftype, [job(10, 152, rank=bed)]) == ERR_ARG
    assert status(lb.decode_frames_list_device, frames, ftype, [job(5, 288, rank=bed)]) == 0
    assert status(lb.decode_frames_biterr_device, frames, ftype, [job(8, 432, biterr=bed)]) == ERR_ARG
    assert status(lb.decode_frames_device, frames, ftype, [job(9, 288)]) == ERR_SIZE
    assert status(lb.decode_frames_device, frames, ftype, [job(9, 300)]) == ERR_ALIGN
    assert status(lb.decode_frames_device, frames, ftype, [job(9, 296, frame_scramb=None)]) == ERR_ARG
    assert status(lb.decode_frames_device, frames, ftype, [job(9 | lb.JOB_RM3014, 296)]) == ERR_ARG
    torch.cuda.synchronize()
