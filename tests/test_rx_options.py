"""The receive chain's create flags taken together, on the CPU: the rule of the accepted subsets, the preconditions of the stream the GPU
matrix runs (tests/test_rx_options_gpu.py) -- every option changes something there, and where options meet they change each other's
rows --, and the fixture tests/golden/rx_options_golden.npz against the host pipeline (tests/options_pipeline.py) that wrote it."""
import os

import numpy as np
import pytest

from tests import chain_host as ch
from tests import list_pipeline as LP
from tests import options_pipeline as OP
from tests.options_pipeline import AACH_RM3014, AACH_SOFT, LIST, SOFT, SYNC_TOLERANT

ROUTES = [(tol, soft) for tol in (0, SYNC_TOLERANT) for soft in (0, SOFT)]


def _ref_built():
    from oracle import ref_binding
    return ref_binding.available() and ref_binding.lmac_available()


@pytest.fixture(scope="module")
def want():
    """(bits, {class: expectation}) from the pipeline where oracle/_ref is built, else from the fixture"""
    if _ref_built():
        from tests.golden import make_rx_options_golden as G
        return G.make()
    return OP.load_golden()


def test_accepted_subsets_and_row_classes():
    """80 of the 128 subsets are accepted: AACH_SOFT needs SOFT and excludes AACH_RM3014.  They are the 20 row classes times BITERR and
    ONE_STREAM."""
    sets = OP.subsets()
    assert len(sets) == len(set(sets)) == 128
    ok = [f for f in sets if OP.accepted(f)]
    assert len(ok) == 80 and len(OP.classes()) == 20 and 0 in OP.classes()
    assert sorted(ok) == sorted(c | b | o for c in OP.classes() for b in (0, OP.BITERR) for o in (0, OP.ONE_STREAM))
    refused = [f for f in sets if not OP.accepted(f)]
    assert len(refused) == 48 and all(f & AACH_SOFT and (not f & SOFT or f & AACH_RM3014) for f in refused)
    assert len({OP.class_name(c) for c in OP.classes()}) == 20
    assert not any(OP.accepted(f | bad) for f in ok for bad in OP.UNDEFINED_BITS)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tetra_rx.h")).read()
    for name, v in (("ONE_STREAM", OP.ONE_STREAM), ("AACH_RM3014", AACH_RM3014), ("SOFT", SOFT), ("BITERR", OP.BITERR),
                    ("SYNC_TOLERANT", SYNC_TOLERANT), ("LIST", LIST), ("AACH_SOFT", AACH_SOFT)):
        assert "TETRA_RX_FLAG_%s = %d" % (name, v) in hdr, name


def _bbk(rows):
    return {k: v for k, v in rows.items() if k[0] == ch.KIND_BBK}


def _coded(rows):
    return {k: v for k, v in rows.items() if k[0] != ch.KIND_BBK}


def _behind_rescued_sb1(with_list, key):
    return any(k[0] == ch.KIND_SB1 and v[4] > 0 and k[1] == key[1] and k[2] <= key[2] for k, v in _coded(with_list).items())


def test_every_option_changes_something_on_the_chosen_stream(want):
    """From the pipeline alone: the tolerant rule reports more frames on at least two channels; on each (synchroniser, hard / soft) route
    four candidates rescue rows that none leaves CRC-bad and lose none, and on both hard routes a rescued SB1 gives a later block another
    verdict, other bits or another time; behind a rescued SB1 an AACH row has other bits, another verdict or another distance under the
    Reed-Muller rule and under maximum likelihood; the Reed-Muller rule corrects rows and refuses rows, maximum likelihood accepts rows it
    refuses; and list decoding changes a channel's link figures."""
    bits, w = want
    n_ch = len(bits)
    frames = {tol: [sum(1 for k in _bbk(w[tol]["rows"]) if k[1] == c) for c in range(n_ch)] for tol in (0, SYNC_TOLERANT)}
    print("frames per channel: reference rule %s, tolerant rule %s" % (frames[0], frames[SYNC_TOLERANT]))
    assert sum(t > r for r, t in zip(frames[0], frames[SYNC_TOLERANT])) >= 2
    changed = {"rm": 0, "ml": 0}
    for tol, soft in ROUTES:
        on, off = _coded(w[tol | soft | LIST]["rows"]), _coded(w[tol | soft]["rows"])
        rescued = [k for k in on if on[k][4] > 0]
        matters = LP.rescued_sb1_matters(on, off)
        unrescued = sum(1 for k in on if on[k][4] <= 0 and on[k][:4] != off[k][:4])
        links = sum(a != b for a, b in zip(w[tol | soft | LIST]["links"], w[tol | soft]["links"]))
        line = "%-13s rows %d, CRC-bad without list %d, rescued %d (SB1 %d), rescued SB1 matters %s, rows not rescued themselves that differ %d, " \
               "channels with other link figures %d" % (OP.class_name(tol | soft)[:-11], len(on), sum(1 for v in off.values() if not v[0]), len(rescued),
                                                         sum(1 for k in rescued if k[0] == ch.KIND_SB1), matters, unrescued, links)
        assert set(on) == set(off) and all(on[k][0] >= off[k][0] for k in on)
        assert len(rescued) >= 1 and all(off[k][0] == 0 and on[k][0] == 1 for k in rescued)
        assert all(v[4] == (0 if v[0] else -1) for v in off.values())
        assert matters or soft
        assert links >= 1
        for rule, flag in (("rm", AACH_RM3014),) + ((("ml", AACH_SOFT),) if soft else ()):
            a, b = _bbk(w[tol | soft | LIST | flag]["rows"]), _bbk(w[tol | soft | flag]["rows"])
            assert set(a) == set(b)
            diff = [k for k in a if (a[k][0], a[k][3], a[k][4]) != (b[k][0], b[k][3], b[k][4])]
            assert all(_behind_rescued_sb1(w[tol | soft | LIST]["rows"], k) for k in diff)
            changed[rule] += len(diff)
            line += ", AACH rows a rescue changes under %s %d" % (rule, len(diff))
        print(line)
    assert changed["rm"] >= 1 and changed["ml"] >= 1
    for tol, soft in ROUTES:
        for lst in (0, LIST):
            rm = _bbk(w[tol | soft | lst | AACH_RM3014]["rows"])
            plain = _bbk(w[tol | soft | lst]["rows"])
            corrected = [k for k, v in rm.items() if v[4] in (1, 2, 3)]
            refused = [k for k, v in rm.items() if v[4] == 0xff]
            assert all(rm[k][0] == 1 and rm[k][3] != plain[k][3] for k in corrected) and all(rm[k][0] == 0 and rm[k][3] == plain[k][3] for k in refused)
            assert all(v[0] == 1 and v[4] is None and v[5] is None for v in plain.values())
            line = "%-18s AACH rows %d: Reed-Muller corrects %d, refuses %d" % (OP.class_name(tol | soft | lst)[:-5], len(rm), len(corrected), len(refused))
            assert len(corrected) >= 1 and len(refused) >= 1
            if soft:
                ml = _bbk(w[tol | soft | lst | AACH_SOFT]["rows"])
                kept = [k for k in refused if ml[k][0] == 1]
                line += ", maximum likelihood accepts %d of those" % len(kept)
                assert len(kept) >= 1 and all(v[5] >= 1 for v in ml.values() if v[0]) and all(v[5] == 0 for v in ml.values() if not v[0])
            print(line)
    assert all(len(x["cells"]) == n_ch and all(c[0] != 0 for c in x["cells"]) for x in w.values())          # every channel ends with a cell's code


def test_fixture_is_the_host_pipeline(want):
    """tests/golden/rx_options_golden.npz is what tests/golden/make_rx_options_golden.py makes from oracle/_ref, stays small, and its
    arrays give back the expectations they were made from."""
    assert os.path.getsize(OP.GOLDEN) < 300 * 1024
    g = OP.load_golden()
    assert sorted(g[1]) == OP.classes() and len(g[0]) == len(OP.SEEDS)
    assert OP.same(OP.from_arrays(OP.to_arrays(*g)), g)
    if not _ref_built():
        pytest.skip("oracle/_ref not built and the reference not present: the fixture stands alone")
    assert OP.same(g, want)
    again, stored = OP.to_arrays(*want), np.load(OP.GOLDEN)
    assert set(again) == set(stored.files) and all(np.array_equal(again[k], stored[k]) for k in again)
