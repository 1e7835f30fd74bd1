"""TCH/4.8 and TCH/2.4 interleaved over N = 1, 4 or 8 blocks (include/ext/tetra_tch_nblk.h) on the GPU: the device entry points
(k_tch_nblk, k_tch_nblk_soft), the host-pointer variants and the refusals.  Expected rows and counts are the definition's
(tests/tch_nblk_definition.py): from oracle/_ref where it is built, else from tests/golden/lmac_tch_nblk_golden.npz, which
tests/test_lmac_tch_nblk.py holds against the definition whenever the reference is at hand.  Every output is poisoned before a launch;
everything is integer and every comparison exact."""
import numpy as np
import pytest

from tests import tch_nblk_definition as nd

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_ALIGN = -1, -7                        # include/tetra_demod.h
SENTINEL = 0x5a5a5a5a
MODES = ("hard", "soft")
DEPTHS = (1,) + nd.NS


@pytest.fixture(scope="module")
def want():
    """Read-only: the pools, code tables, window tables, want_* and be_* of tests/tch_nblk_definition.py."""
    from oracle import ref_binding
    if ref_binding.available() and ref_binding.lmac_available():
        from tests.golden import make_lmac_tch_nblk_golden as G
        z = G.make(ref_binding.lmac_lib())
        print("expected values from oracle/_ref")
    else:
        z = dict(nd.load_golden())
        print("expected values from tests/golden/lmac_tch_nblk_golden.npz")
    for a in z.values():
        a.flags.writeable = False
    return z


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _u32(torch, a, dev):
    return torch.from_numpy(np.array(a, np.uint32).view(np.int32)).to(dev)          # (a copy: the pools are read-only)


def _case(want, kind, n, mode):
    tag = dict(nd.cases(kind))[n]
    return (want[mode + "_" + tag], want["table_" + tag], want["index_" + tag], want["win_%d_%d" % (kind, n)],
            want["want_%s_%d_%d" % (mode, kind, n)], want["be_%s_%d_%d" % (mode, kind, n)])


def nblk_call(pkg, kind, n, mode, pool, table, index, win, have=None, stride=432, counts=True, capacity=None):
    """tetra_lmac_decode_tch_nblk[_soft]_device on `pool` ([m][432]) laid `stride` apart with junk between the rows -> (type2 rows with
    their padding of 8, count words or None), outputs poisoned with 7 / SENTINEL.  capacity: n_blocks as the entry is told it."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    n2 = nd.BLK[kind][1]
    ost = n2 + 8
    laid = np.full((len(pool), stride), 0x77, pool.dtype)
    laid[:, :432] = pool
    cap = len(win) if capacity is None else capacity
    t2 = torch.full((max(cap, 1), ost), 7, dtype=torch.uint8, device=dev)
    be = _u32(torch, np.full(max(cap, 1), SENTINEL), dev) if counts else None
    entry = lb.decode_tch_nblk_soft_device if mode == "soft" else lb.decode_tch_nblk_device
    entry(kind, n, torch.from_numpy(laid).to(dev), len(pool), stride, _u32(torch, table, dev),
          None if index is None else torch.from_numpy(np.array(index, np.int32)).to(dev), torch.from_numpy(np.array(win, np.int32)).to(dev), cap,
          None if have is None else torch.tensor([have], dtype=torch.int32, device=dev), t2, ost, be)
    torch.cuda.synchronize()
    return t2.cpu().numpy(), None if be is None else be.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", DEPTHS)
@pytest.mark.parametrize("kind", nd.CODED)
def test_device_entries_equal_the_definition(pkg, want, kind, n, mode):
    """Every window of the table (at N = 4 and 8 four workgroups, the last one ragged; the first one of complete plain windows), tight
    rows and rows 436 and 448 bytes apart with junk between, codes per row and through the init index, with and without counts; the
    padding behind every output row stays as it was."""
    pool, table, index, win, w, wbe = _case(want, kind, n, mode)
    n2 = nd.BLK[kind][1]
    for stride in (432, 436, 448):
        for counts in (True, False):
            codes, idx = (table, index) if stride != 448 else (table[index], None)
            got, be = nblk_call(pkg, kind, n, mode, pool, codes, idx, win, stride=stride, counts=counts)
            bad = np.flatnonzero((got[:, :n2] != w).any(axis=1))
            assert not len(bad), (kind, n, mode, stride, counts, bad[:8])
            assert be is None or np.array_equal(be, wbe), (kind, n, mode, stride)
            assert (got[:, n2:] == 7).all(), (kind, n, mode, stride, counts)
    assert w.any() and len(set(wbe.tolist())) > 10


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", nd.CODED)
def test_device_side_count_at_the_workgroup_edge(pkg, want, kind, mode):
    """d_n_blocks of 0, 1, 63, 64, 65 and above n_blocks: blocks below the count are the definition's, blocks from the count on keep their
    poison, and so does the padding behind every row."""
    n2 = nd.BLK[kind][1]
    for n in nd.NS:
        pool, table, index, win, w, wbe = _case(want, kind, n, mode)
        # the shuffled half of the table: lost and arbitrary windows in every workgroup
        s = nd.windows_of(n)[1]["shuffled"].start
        win, w, wbe = win[s:s + 130], w[s:s + 130], wbe[s:s + 130]
        for cap, have in ((130, 0), (130, 1), (130, 63), (64, 64), (130, 64), (130, 65), (100, 500), (1, 1)):
            upto = min(cap, have)
            for counts in (True, False):
                got, be = nblk_call(pkg, kind, n, mode, pool, table, index, win[:cap], have=have, counts=counts, capacity=cap)
                assert np.array_equal(got[:upto, :n2], w[:upto]), (kind, n, mode, cap, have)
                assert (got[upto:] == 7).all() and (got[:, n2:] == 7).all(), (kind, n, mode, cap, have)
                if counts:
                    assert np.array_equal(be[:upto], wbe[:upto]) and (be[upto:] == SENTINEL).all(), (kind, n, mode, cap, have)


@pytest.mark.parametrize("kind", nd.CODED)
def test_forced_byte_route_equals_the_packed_route(pkg, want, kind):
    """The first workgroup of every table is entitled to the packed route; with tetra_lmac_debug_force_byte_route it takes the class
    route: the same rows and counts, the definition's."""
    lb = pkg.lmac_binding
    n2 = nd.BLK[kind][1]
    for n in nd.NS:
        pool, table, index, win, w, wbe = _case(want, kind, n, "hard")
        assert win[:64].min() >= 0 and (pool[np.unique(win[:64])] <= 1).all()
        a = nblk_call(pkg, kind, n, "hard", pool, table, index, win[:64])
        old = lb.force_byte_route(True)
        try:
            b = nblk_call(pkg, kind, n, "hard", pool, table, index, win[:64])
            c = nblk_call(pkg, kind, n, "hard", pool, table, index, win)
        finally:
            lb.force_byte_route(old)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.array_equal(a[0][:, :n2], w[:64]) and np.array_equal(a[1], wbe[:64])
        assert np.array_equal(c[0][:, :n2], w) and np.array_equal(c[1], wbe)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", nd.CODED)
def test_host_entries(pkg, want, kind, mode):
    """tetra_lmac_decode_tch_nblk[_soft]_batch through decode_tch_nblk: what the device entries give, padded input rows included."""
    lb = pkg.lmac_binding
    for n in DEPTHS:
        pool, table, index, win, w, wbe = _case(want, kind, n, mode)
        out, be = lb.decode_tch_nblk(kind, n, pool, win, table[index], soft=mode == "soft", biterr=True)
        assert out.shape == w.shape and np.array_equal(out, w) and np.array_equal(be, wbe), (kind, n, mode)
        err, cmp_ = lb.split_biterr(be)
        assert (cmp_ <= 432).all() and (err <= cmp_).all()
        wide = np.full((len(pool), 440), 0x11, pool.dtype)
        wide[:, :432] = pool
        assert np.array_equal(lb.decode_tch_nblk(kind, n, wide, win[:70], table[index], soft=mode == "soft"), w[:70])
    assert lb.decode_tch_nblk(kind, 4, pool, np.zeros((0, 4), np.int32), table[index], soft=mode == "soft").shape == (0, nd.BLK[kind][1])


def test_no_blocks_and_refusals_write_nothing(pkg, want):
    """n_blocks == 0 launches nothing.  TETRA_ERR_ARG for TCH/7.2 and other kinds, for N outside {1, 4, 8}, for NULL windows, pool, codes
    or output, for rows shorter than the block; TETRA_ERR_ALIGN for pointers and strides off the 4-byte grid: every output keeps its
    poison.  The same call is then accepted as it stands."""
    torch, dev = _dev()
    lb = pkg.lmac_binding
    L = lb._lib()
    kind, n = 9, 4
    pool, table, index, win, w, wbe = _case(want, kind, n, "hard")
    spool = _case(want, kind, n, "soft")[0]
    stride = 440
    laid = np.full((len(pool), stride), 0x77, np.uint8)
    laid[:, :432] = pool
    slaid = np.full((len(pool), stride), 0x77, np.int8)
    slaid[:, :432] = spool
    nb = 70
    d_pool, d_soft = torch.from_numpy(laid).to(dev), torch.from_numpy(slaid).to(dev)
    d_codes, d_index = _u32(torch, table, dev), torch.from_numpy(np.array(index, np.int32)).to(dev)
    d_win = torch.from_numpy(np.concatenate([np.array(win[:nb], np.int32).ravel(), np.zeros(4, np.int32)])).to(dev)
    t2 = torch.full((nb, 300), 7, dtype=torch.uint8, device=dev)
    be = _u32(torch, np.full(nb + 1, SENTINEL), dev)
    r, s, i, wp, o, b = d_pool.data_ptr(), d_codes.data_ptr(), d_index.data_ptr(), d_win.data_ptr(), t2.data_ptr(), be.data_ptr()
    m = len(pool)
    for f, r in ((L.tetra_lmac_decode_tch_nblk_device, d_pool.data_ptr()), (L.tetra_lmac_decode_tch_nblk_soft_device, d_soft.data_ptr())):
        assert f(kind, n, r, m, stride, s, i, wp, 0, None, o, 300, b, None) == 0           # no blocks: a no-op
        assert f(kind, n, None, m, stride, None, None, None, 0, None, None, 300, None, None) == 0
        for bad_kind in (8, 5, 11, 9 | 0x100):
            assert f(bad_kind, n, r, m, stride, s, i, wp, nb, None, o, 300, b, None) == ERR_ARG, bad_kind
        for bad_n in (0, 2, 3, 5, 7, 16, -4):
            assert f(kind, bad_n, r, m, stride, s, i, wp, nb, None, o, 300, b, None) == ERR_ARG, bad_n
        assert f(kind, n, r, m, stride, s, i, None, nb, None, o, 300, b, None) == ERR_ARG
        assert f(kind, n, None, m, stride, s, i, wp, nb, None, o, 300, b, None) == ERR_ARG
        assert f(kind, n, r, m, stride, None, i, wp, nb, None, o, 300, b, None) == ERR_ARG
        assert f(kind, n, r, m, stride, s, i, wp, nb, None, None, 300, b, None) == ERR_ARG
        assert f(kind, n, r, -1, stride, s, i, wp, nb, None, o, 300, b, None) == ERR_ARG
        assert f(kind, n, r, m, stride, s, i, wp, -1, None, o, 300, b, None) == ERR_ARG
        assert f(kind, n, r, m, 428, s, i, wp, nb, None, o, 300, b, None) == ERR_ARG         # rows shorter than the block
        assert f(kind, n, r, m, stride, s, i, wp, nb, None, o, 288, b, None) == ERR_ARG
        assert f(kind, n, r + 2, m, stride, s, i, wp, nb, None, o, 300, b, None) == ERR_ALIGN
        assert f(kind, n, r, m, 438, s, i, wp, nb, None, o, 300, b, None) == ERR_ALIGN
        assert f(kind, n, r, m, stride, s, i, wp + 2, nb, None, o, 300, b, None) == ERR_ALIGN
        assert f(kind, n, r, m, stride, s, i, wp, nb, None, o + 1, 300, b, None) == ERR_ALIGN
        assert f(kind, n, r, m, stride, s, i, wp, nb, None, o, 298, b, None) == ERR_ALIGN
        assert f(kind, n, r, m, stride, s, i, wp, nb, None, o, 300, b + 2, None) == ERR_ALIGN
        torch.cuda.synchronize()
        assert (t2 == 7).all() and (be.cpu().numpy().view(np.uint32) == SENTINEL).all(), "a refused call wrote"
    # the same table is accepted as it stands
    assert L.tetra_lmac_decode_tch_nblk_device(kind, n, d_pool.data_ptr(), m, stride, s, i, wp, nb, None, o, 300, b, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(t2.cpu().numpy()[:, :292], w[:nb]) and (t2[:, 292:] == 7).all()
    got = be.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:nb], wbe[:nb]) and got[nb] == SENTINEL
    # the host-pointer variants refuse the same before they touch the device
    for f, rows, w in ((L.tetra_lmac_decode_tch_nblk_batch, laid, w), (L.tetra_lmac_decode_tch_nblk_soft_batch, slaid, _case(want, kind, n, "soft")[4])):
        out = np.full((nb, 292), 7, np.uint8)
        hw, hc = np.array(win[:nb], np.int32), np.array(table[index], np.uint32)
        args = lambda k, d, w_=hw: (k, d, rows.ctypes.data, m, stride, hc.ctypes.data, None if w_ is None else w_.ctypes.data, nb, out.ctypes.data, 292, None, -1)
        assert f(*args(8, 4)) == ERR_ARG and f(*args(9, 2)) == ERR_ARG and f(*args(9, 4, None)) == ERR_ARG
        assert (out == 7).all()
        assert f(*args(9, 4)) == 0 and np.array_equal(out, w[:nb])
