"""Every accepted set of the receive chain's seven create flags against ONE host pipeline (tests/options_pipeline.py): the 20 row classes
(synchroniser rule x hard / soft x list decoding x AACH rule), each with BITERR off and on and on two streams and one, so all 80 accepted
subsets run, flag set 0 among them; and the refusals over all 128 subsets.  Expected values come from oracle/_ref where it is built, else
from tests/golden/rx_options_golden.npz, which tests/test_rx_options.py holds against the pipeline wherever the reference is at hand.
Everything is integer and every comparison exact."""
import ctypes as C

import numpy as np
import pytest

from tests import chain_host as ch
from tests import options_pipeline as OP
from tests.chain_gpu import run_calls
from tests.options_pipeline import AACH_RM3014, AACH_SOFT, BITERR, LIST, ONE_STREAM, SOFT, SYNC_TOLERANT

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_UNSUPPORTED = -1, -2                # include/tetra_demod.h


@pytest.fixture(scope="module")
def want():
    """Read-only: (the oracle demodulator's bits per channel, {class flags: expectation})."""
    from oracle import ref_binding
    if ref_binding.available() and ref_binding.lmac_available():
        from tests.golden import make_rx_options_golden as G
        print("expected values from oracle/_ref")
        return G.make()
    print("expected values from tests/golden/rx_options_golden.npz")
    return OP.load_golden()


@pytest.fixture(scope="module")
def iq(synth):
    out = OP.stream_iq(synth)
    out.flags.writeable = False
    return out


@pytest.fixture(scope="module")
def misses_seen():
    """sync_misses() of every handle so far, by synchroniser rule"""
    return {}


def _refuses(pkg, fn):
    with pytest.raises(pkg.TetraDemodError) as e:
        fn()
    return e.value.status == ERR_UNSUPPORTED


def run_handle(pkg, iq, flags):
    """The stream in OP.CUTS' ragged calls through one handle; after every call every kind is fetched with every column the flag set has.
    -> dict: rows {(kind, channel, bitnum): tuple in the pipeline's form, None for a column the flag set lacks}, the chain's bits, cells,
    links (None without BITERR), misses.  Behind the last call: the accessors of the flags not set refuse, and one extended delivery per
    which = 0 / 1 gives the rows and columns the fetches of those calls gave."""
    R = pkg.rx_binding
    rows, calls = {}, []
    aach = flags & (AACH_RM3014 | AACH_SOFT)

    def per_call(rx, i, s):
        got = {}
        for k in range(R.N_KINDS):
            blocks, t1 = rx.fetch(k)
            cols = {}
            if k == R.KIND_BBK:
                if aach:
                    cols["aach_dist"] = rx.fetch_aach_dist()
                if flags & AACH_SOFT:
                    cols["margin"] = rx.fetch_aach_margin()
            else:
                if flags & LIST:
                    cols["rank"] = rx.fetch_list_rank(k)
                if flags & BITERR:
                    cols["biterr"] = rx._count_then_fetch(rx._lib.tetra_rx_fetch_biterr, np.uint32, 0, k)
                    err, cmp_ = rx.fetch_biterr(k)
                    assert np.array_equal(err, cols["biterr"] & 0xffff) and np.array_equal(cmp_, cols["biterr"] >> 16)
            assert all(len(c) == len(blocks) for c in cols.values()), (flags, i, k)
            got[k] = (blocks.copy(), t1.copy(), {n: c.copy() for n, c in cols.items()})
            for j, b in enumerate(blocks):
                key = (k, int(b["channel"]), int(b["bitnum"]))
                assert key not in rows, (flags, key)
                head = (int(b["crc_ok"]), int(b["tdma_time_rx"]), int(b["tdma_time"]), t1[j].tobytes())
                if k == R.KIND_BBK:
                    rows[key] = head + (int(cols["aach_dist"][j]) if aach else None, int(cols["margin"][j]) if flags & AACH_SOFT else None)
                else:
                    rows[key] = head + (int(cols["rank"][j]) if flags & LIST else None,
                                        (int(cols["biterr"][j]) & 0xffff, int(cols["biterr"][j]) >> 16) if flags & BITERR else None)
        calls.append(got)

    def after(rx):
        out = dict(links=rx.links() if flags & BITERR else None, misses=[int(m) for m in rx.sync_misses()])
        k = R.KIND_SCH_F
        if not flags & LIST:
            assert _refuses(pkg, lambda: rx.fetch_list_rank(k)) and _refuses(pkg, lambda: rx.set_list_candidates(4)) and _refuses(pkg, lambda: rx.list_rank_device(k))
            assert _refuses(pkg, lambda: rx.out_bound(extras=R.EXT_ROW_LIST_RANK))
        if not flags & BITERR:
            assert _refuses(pkg, lambda: rx.fetch_biterr(k)) and _refuses(pkg, rx.links) and _refuses(pkg, lambda: rx.biterr_device(k))
            assert _refuses(pkg, lambda: rx.out_bound(extras=R.EXT_ROW_BITERR)) and _refuses(pkg, lambda: rx.out_bound(extras=R.EXT_CHAN_LINK))
        if not aach:
            assert _refuses(pkg, rx.fetch_aach_dist) and _refuses(pkg, lambda: rx.out_bound(extras=R.EXT_ROW_AACH_DIST))
        if not flags & AACH_SOFT:
            assert _refuses(pkg, rx.fetch_aach_margin) and _refuses(pkg, lambda: rx.set_aach_min_margin(5))
        extras = (R.EXT_ROW_BITERR if flags & BITERR else 0) | (R.EXT_ROW_LIST_RANK if flags & LIST else 0) | (R.EXT_ROW_AACH_DIST if aach else 0)
        for which in (0, 1):
            d = rx.deliver(which, extras=extras)
            dl = d.wait()
            assert d.header.call == len(calls) - 1 - which and (not extras or d.ext_header.extras == extras), (flags, which)
            for kind, (blocks, t1, cols) in calls[-1 - which].items():
                assert dl[kind][0].tobytes() == blocks.tobytes() and np.array_equal(dl[kind][1][:, :t1.shape[1]], t1), (flags, which, kind)
                for name in ("biterr", "rank", "aach_dist"):
                    col = dl.columns[kind][name] if extras else None
                    assert (col is None) == (name not in cols) and (col is None or np.array_equal(col, cols[name])), (flags, which, kind, name)
        return out

    bits, cells, out = run_calls(pkg, iq, OP.CUTS, flags, per_call, after=after)
    assert len(calls) == len(OP.CUTS) - 1 >= 3
    out.update(rows=rows, bits=bits, cells=[tuple(int(v) for v in np.frombuffer(c, np.uint32)) for c in cells])
    return out


@pytest.mark.parametrize("cls", OP.classes(), ids=OP.class_name)
def test_chain_equals_the_pipeline_under_every_flag_set_of_the_class(pkg, iq, want, misses_seen, cls):
    """Four handles of one row class -- BITERR off / on, two streams / ONE_STREAM -- fed the stream in five ragged calls.  Per handle: the
    chain's own bits are the oracle demodulator's; every row of every kind, keyed (kind, channel, bit number), is the pipeline's with none
    missing or extra: verdict, both times, type-1 bits, the rank under LIST, the count under BITERR, the AACH distance under either AACH
    flag and its margin under AACH_SOFT; links() and cells() are the pipeline's; the miss counters are the restatement's and equal across
    the handles of one synchroniser rule; accessors of flags not set refuse; the delivery carries the fetches' columns."""
    bits, expect = want
    w = expect[cls]
    n_kind = None
    for extra in (0, BITERR, ONE_STREAM, BITERR | ONE_STREAM):
        flags = cls | extra
        got = run_handle(pkg, np.array(iq), flags)
        assert len(got["bits"]) == len(bits) and all(np.array_equal(a, b) for a, b in zip(got["bits"], bits)), flags
        rows = got["rows"]
        missing, surplus = sorted(set(w["rows"]) - set(rows)), sorted(set(rows) - set(w["rows"]))
        assert not missing and not surplus, (flags, missing[:5], surplus[:5])
        for key, v in w["rows"].items():
            g = rows[key]
            if key[0] == ch.KIND_BBK:
                assert g == v, (flags, key, g[:3], v[:3], g[4:], v[4:])
            else:
                assert g[:4] == v[:4], (flags, key, g[:3], v[:3])
                assert not flags & LIST or g[4] == v[4], (flags, key, g[4], v[4])
                assert not flags & BITERR or g[5] == v[5], (flags, key, g[5], v[5])
        assert got["cells"] == w["cells"], (flags, got["cells"], w["cells"])
        assert got["links"] == (w["links"] if flags & BITERR else None), (flags, got["links"], w["links"])
        assert got["misses"] == w["misses"] == misses_seen.setdefault(cls & SYNC_TOLERANT, got["misses"]), (flags, got["misses"], w["misses"])
        n_kind = [sum(1 for k in rows if k[0] == kind) for kind in range(6)]
    print("%s: rows compared per handle %s (SB1, BBK, SB2, NDB1, NDB2, SCH/F), CRC-good %d, rescued %d" %
          (OP.class_name(cls), n_kind, sum(v[0] for v in w["rows"].values()), sum(1 for k, v in w["rows"].items() if k[0] != ch.KIND_BBK and v[4] > 0)))
    assert sum(n_kind) == len(w["rows"]) >= 100


def _create(R, flags):
    """tetra_rx_create on a small configuration -> (status, handle value); the handle pointer is poisoned beforehand"""
    L = R._lib()
    cfg = R.RxConfig()
    assert L.tetra_rx_default_config(C.byref(cfg)) == 0
    cfg.demod.n_channels, cfg.demod.max_samples, cfg.demod.device, cfg.flags = 2, 2000, -1, flags
    h = C.c_void_p(0xdead0)
    rc = L.tetra_rx_create(C.byref(cfg), C.byref(h))
    return rc, h


def test_create_accepts_exactly_the_80_subsets(pkg):
    """All 128 subsets of the seven flag bits: a handle exactly for the 80 of options_pipeline.accepted, TETRA_ERR_ARG and no handle for
    the other 48; and each undefined low bit -- 4, 16, 64, 256, 2048 -- beside any accepted subset is refused."""
    R = pkg.rx_binding
    assert [R.FLAG_ONE_STREAM, R.FLAG_AACH_RM3014, R.FLAG_SOFT, R.FLAG_BITERR, R.FLAG_SYNC_TOLERANT, R.FLAG_LIST, R.FLAG_AACH_SOFT] == list(OP.FLAG_BITS)
    made = refused = 0
    for flags in OP.subsets():
        rc, h = _create(R, flags)
        if OP.accepted(flags):
            assert rc == 0 and h.value not in (None, 0xdead0), flags
            assert R._lib().tetra_rx_destroy(h) == 0
            made += 1
            for bad in OP.UNDEFINED_BITS:
                rc, h = _create(R, flags | bad)
                assert rc == ERR_ARG and h.value is None, (flags, bad)
        else:
            assert rc == ERR_ARG and h.value is None, flags
            refused += 1
    assert (made, refused) == (80, 48)
