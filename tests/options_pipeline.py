"""What the receive chain has to give under ANY accepted set of its seven create flags, stated once on the host by composing the pipelines
the single options are pinned to -- for tests/test_rx_options.py (CPU) and tests/test_rx_options_gpu.py (the matrix on the GPU):

    frames        oracle.BurstSyncOracle, under SYNC_TOLERANT tests/test_sync_tol.Restatement(ref, DEFAULT)
    coded kinds   tests/list_pipeline.channel_walk (the numpy decoder of tests/list_definition.py, T = 0 without LIST and 4 with it, on the
                  oracle demodulator's bits or, under SOFT, on the quantised oracle symbols), SB1 first and feeding tests/chain_host.walk
    AACH          per frame of that walk the 30 positions under the code in force behind the burst's SB1 (rescued ones included): handed on,
                  or the radius-3 rule of include/tetra_aach.h by brute force over the recorded codewords (aach_soft_pipeline.hard_rm), or
                  tests/aach_soft_definition.py's maximum likelihood on the sign-descrambled soft values at min_margin 1
    link figures  tests/test_biterr._link_sums' rule over the pipeline's own coded rows
    cell          the walk's last code, the last good SYNC PDU's identity and time, and the clock behind the last frame

ONE_STREAM and BITERR change no row, so the distinct expectations are the 20 classes (synchroniser, soft, list, AACH rule).  Nothing of
the product's code runs here beyond what tests/chain_host.py names (host_clock)."""
import itertools
import os

import numpy as np

from tests import aach_soft_definition as A
from tests import aach_soft_pipeline as AP
from tests import chain_host as ch
from tests import list_definition as D
from tests import list_pipeline as LP

# include/tetra_rx.h
ONE_STREAM, AACH_RM3014, SOFT, BITERR, SYNC_TOLERANT, LIST, AACH_SOFT = 1, 2, 8, 32, 128, 512, 1024
FLAG_BITS = (ONE_STREAM, AACH_RM3014, SOFT, BITERR, SYNC_TOLERANT, LIST, AACH_SOFT)
UNDEFINED_BITS = (4, 16, 64, 256, 2048)          # the low bits that are no flag
ROW_CLASS_MASK = AACH_RM3014 | SOFT | SYNC_TOLERANT | LIST | AACH_SOFT          # the flags that change rows
LIST_T = 4                                       # TETRA_LIST_DEFAULT_CANDIDATES

# The stream: four downlinks of tests/test_list_chain.py's recipe with RM-coded AACHs, one per seed.  The seeds were chosen on the CPU,
# from this pipeline alone, so that every option changes something (tests/test_rx_options.py asserts it and prints the counts).  Of the
# seeds 0 .. 799, each taken as a channel of its own: 213 and 215 have a rescued SB1 that matters on both hard routes but none that
# changes an AACH row (nor have 180, 198, 211, 271, 278, 292, which also have rescued rows on all four routes); a rescued SB1 changes
# AACH rows under the Reed-Muller rule on a hard route for 1, 73, 102, 105, 106, 143, 152, 153, 161, 248, 249, 289, 294, 326, 399, 457,
# 539, 541, 564, 605, 717, 725, 739, and on a soft route -- there under maximum likelihood too -- for 4, 13, 25, 53, 79, 119, 143, 160,
# 267, 309, 350, 359, 376, 428, 440, 509, 520, 547, 607, 651, 742.  Of those in 180 .. 299, 249 is the first on the reference
# synchroniser's hard route and 267 the first on a soft route.  (On seed 326 a rescued SB1 costs a later block its CRC: "no row is lost"
# does not hold there.)
SAMPLES, SLOTS, ESN0 = 18000, 36, 11.0
SEEDS = (213, 215, 249, 267)
CUTS = (0, 9000, 9180, 9181, 13181, SAMPLES)     # five ragged calls
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rx_options_golden.npz")


def accepted(flags):
    """tetra_rx_create's rule: only the seven flag bits, and AACH_SOFT reads the soft ring and excludes the other AACH decoder"""
    if flags & ~sum(FLAG_BITS):
        return False
    return not (flags & AACH_SOFT) or bool(flags & SOFT) and not (flags & AACH_RM3014)


def subsets():
    """all 128 subsets of the seven flag bits"""
    return [sum(c) for r in range(len(FLAG_BITS) + 1) for c in itertools.combinations(FLAG_BITS, r)]


def classes():
    """the 20 row classes: the accepted subsets of the flags that change rows"""
    return sorted(f for f in subsets() if accepted(f) and not f & ~ROW_CLASS_MASK)


def class_name(flags):
    aach = "ml" if flags & AACH_SOFT else "rm" if flags & AACH_RM3014 else "pass"
    return "%s_%s_%s_%s" % ("tol" if flags & SYNC_TOLERANT else "ref", "soft" if flags & SOFT else "hard", "list" if flags & LIST else "plain", aach)


def sent_info(seed):
    return np.random.default_rng(seed + 50).integers(0, 16384, SLOTS)


def stream_iq(synth, seeds=SEEDS):
    rows = []
    for s in seeds:
        tx = synth.gen_downlink(SLOTS, 8100 + s, cell=(200 + s % 50, 3000 + s, 9 + s % 40), aach=A.code_bits()[sent_info(s)])
        rows.append(synth.gen_channel(SAMPLES, 8200 + s, bits=tx[0], esn0_db=ESN0)[0])
    return np.stack(rows).astype(np.complex64)


def aach_rows(walk, soft, channel, rule):
    """The AACH of every downlink burst of a walk (list_pipeline.channel_walk's) -> {(KIND_BBK, channel, bitnum): (crc_ok, time on entry,
    time, the 30 bits, dist or None, margin or None)}.  rule: "pass", "rm" (hard bits of the frame) or "ml" (soft: the quantiser's values)."""
    at = [f for f in range(len(walk["types"])) if int(walk["types"][f]) in ch.BURST_KINDS]
    pieces = [ch.BLOCK[(int(walk["types"][f]), ch.KIND_BBK)].pieces for f in at]
    seqs = [D.scramb_seq(int(walk["codes"][f]), 30) for f in at]
    if rule == "ml":
        values = np.array([A.descramble(ch.cut(soft, int(walk["bitnums"][f]), p), s) for f, p, s in zip(at, pieces, seqs)]).reshape(-1, 30)
        rows, ok = A.rows(values, 1)
        bits, dist, margin = rows[:, :30], [int(v) for v in rows[:, 30]], [int(v) for v in rows[:, 31]]
    else:
        hard = np.array([ch.cut(walk["frames"][f], 0, p) ^ s for f, p, s in zip(at, pieces, seqs)], np.uint8).reshape(-1, 30)
        if rule == "rm":
            info, d = AP.hard_rm(hard)
            ok = (d <= 3).astype(np.int32)
            bits = np.where(ok[:, None] != 0, A.code_bits()[np.maximum(info, 0)], hard)
            dist, margin = [int(v) if v <= 3 else 0xff for v in d], [None] * len(at)
        else:
            bits, ok, dist, margin = hard, np.ones(len(at), np.int32), [None] * len(at), [None] * len(at)
    return {(ch.KIND_BBK, channel, int(walk["bitnums"][f])): (int(ok[j]), int(walk["t_rx"][f]), int(walk["t_af"][f]), bits[j].astype(np.uint8).tobytes(),
                                                              dist[j], margin[j]) for j, f in enumerate(at)}


def final_cell(walk):
    """tetra_lmac_cell_state_t's ten fields behind the walk's last frame"""
    code, ident, tcd = 0, (0, 0, 0), (0, 0, 0)
    for f, got in enumerate(walk["sb1"]):
        if got is not None and got[1]:
            mcc, mnc, colour, tn, fn, mn = ch.sync_pdu_fields(got[0])
            code, ident, tcd = int(walk["codes"][f]), (colour, mcc, mnc), (tn, fn, mn)
    t = int(walk["t_af"][-1]) if len(walk["t_af"]) else 0
    return (code,) + ident + tcd + (t & 0xff, (t >> 8) & 0xff, t >> 16)


def link_sums(rows, n_channels):
    """tests/test_biterr._link_sums over the coded rows of a class, handed to it as one call's fetches"""
    from tests.test_biterr import _link_sums
    call = {"biterr": {}}
    for k in ch.CODED_KINDS:
        mine = [(key, v) for key, v in sorted(rows.items()) if key[0] == k]
        blocks = np.zeros(len(mine), [("channel", "<i4"), ("crc_ok", "<i4")])
        blocks["channel"], blocks["crc_ok"] = [key[1] for key, _ in mine], [v[0] for _, v in mine]
        call[k] = (blocks, None)
        call["biterr"][k] = ([v[5][0] for _, v in mine], [v[5][1] for _, v in mine])
    return _link_sums([call], n_channels)


def tolerant_sync(ref):
    from tests.test_sync_tol import DEFAULT, Restatement
    return lambda: Restatement(ref, DEFAULT)


def expectations(ref, oracle, bits, soft):
    """bits, soft: soft_pipeline.oracle_streams' per channel -> {class flags: dict(rows {(kind, channel, bitnum): tuple}, links [per channel],
    cells [per channel], misses [per channel])} for the 20 classes."""
    out = {}
    n_ch = len(bits)
    for tol, use_soft, lst in itertools.product((0, SYNC_TOLERANT), (0, SOFT), (0, LIST)):
        coded, bbk, cells, misses = {}, {"pass": {}, "rm": {}, "ml": {}}, [], []
        for c in range(n_ch):
            made = []

            def sync():
                made.append(tolerant_sync(ref)() if tol else oracle.BurstSyncOracle())
                return made[-1]
            rows, walk = LP.channel_walk(oracle, bits[c], c, LIST_T if lst else 0, soft[c] if use_soft else None, sync)
            coded.update(rows)
            for rule in ("pass", "rm") + (("ml",) if use_soft else ()):
                bbk[rule].update(aach_rows(walk, soft[c], c, rule))
            cells.append(final_cell(walk))
            misses.append(made[0].history[-1][4] if tol else 0)
        links = link_sums(coded, n_ch)
        for rule, aach in (("pass", 0), ("rm", AACH_RM3014), ("ml", AACH_SOFT)):
            if rule != "ml" or use_soft:
                out[tol | use_soft | lst | aach] = dict(rows={**coded, **bbk[rule]}, links=links, cells=cells, misses=misses)
    assert sorted(out) == classes()
    return out


# ---- the fixture: tests/golden/rx_options_golden.npz ----------------------------------------------------------------------------------------
def _pack(rows):
    """rows {key: tuple} -> arrays: key [n][3], label [n][3], bits [n][34] (the type-1 bits packed), extra [n][3] (coded: rank, errors,
    compared; BBK: dist, margin, 0; -2 = None)"""
    keys = sorted(rows)
    bits = np.zeros((len(keys), 272), np.uint8)
    extra = np.zeros((len(keys), 3), np.int64)
    for j, k in enumerate(keys):
        v = rows[k]
        b = np.frombuffer(v[3], np.uint8)
        bits[j, :len(b)] = b
        extra[j] = (-2 if v[4] is None else v[4], -2 if v[5] is None else v[5], 0) if k[0] == ch.KIND_BBK else (v[4], v[5][0], v[5][1])
    return dict(key=np.array(keys, np.int64).reshape(-1, 3), label=np.array([rows[k][:3] for k in keys], np.int64).reshape(-1, 3),
                bits=np.packbits(bits, axis=1), extra=extra)


def _unpack(a):
    rows = {}
    bits = np.unpackbits(a["bits"], axis=1)
    none = lambda v: None if v == -2 else int(v)
    for key, lab, b, e in zip(a["key"], a["label"], bits, a["extra"]):
        k = int(key[0])
        head = tuple(int(x) for x in lab) + (b[:ch.TYPE1_BITS[k]].tobytes(),)
        rows[tuple(int(x) for x in key)] = head + ((none(e[0]), none(e[1])) if k == ch.KIND_BBK else (int(e[0]), (int(e[1]), int(e[2]))))
    return rows


def to_arrays(bits, want):
    """the oracle demodulator's bits and the 20 classes as the fixture's arrays: the coded rows once per (synchroniser, soft, list), the
    AACH rows, the cells and the miss counters; the link figures follow from the rows"""
    out = {"n_bits": np.array([len(b) for b in bits], np.int64), "demod_bits": np.packbits(np.concatenate(bits))}
    for flags, w in want.items():
        name = class_name(flags)
        coded = {k: v for k, v in w["rows"].items() if k[0] != ch.KIND_BBK}
        bbk = {k: v for k, v in w["rows"].items() if k[0] == ch.KIND_BBK}
        for part, rows in (("bbk", bbk),) + ((("coded", coded),) if not flags & (AACH_RM3014 | AACH_SOFT) else ()):
            for field, arr in _pack(rows).items():
                out["%s_%s_%s" % (name, part, field)] = arr
        if not flags & (AACH_RM3014 | AACH_SOFT):
            out[name + "_cells"], out[name + "_misses"] = np.array(w["cells"], np.int64), np.array(w["misses"], np.int64)
    return out


def from_arrays(g):
    """to_arrays inverted -> (bits per channel, {class flags: expectation})"""
    n = [int(v) for v in g["n_bits"]]
    flat = np.unpackbits(g["demod_bits"])
    bits = [flat[sum(n[:c]):sum(n[:c + 1])] for c in range(len(n))]
    want = {}
    for flags in classes():
        name, base = class_name(flags), class_name(flags & ~(AACH_RM3014 | AACH_SOFT))
        coded = _unpack({f: g["%s_coded_%s" % (base, f)] for f in ("key", "label", "bits", "extra")})
        bbk = _unpack({f: g["%s_bbk_%s" % (name, f)] for f in ("key", "label", "bits", "extra")})
        want[flags] = dict(rows={**coded, **bbk}, links=link_sums(coded, len(n)), cells=[tuple(int(x) for x in r) for r in g[base + "_cells"]],
                           misses=[int(x) for x in g[base + "_misses"]])
    return bits, want


def load_golden():
    return from_arrays(np.load(GOLDEN))


def same(a, b):
    """two (bits, expectations) are the same"""
    return len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]
