"""Writes tests/golden/lmac_soft_golden.npz: what the REFERENCE's own soft chain (tests/soft_pipeline.ref_soft_decode: sign-descramble ->
block_deinterleave -> tetra_rcpc_depunct -> conv_cch_decode -> crc16_ccitt_bits of oracle/_ref) answers on the planted inputs of
tests/test_lmac_soft_gpu.py, for a machine without the reference.  The inputs are made again from their seeds by the test (planted(),
list_rows() below); the file holds a checksum of them, and per kind the reference's type-2 bits (np.packbits) and verdicts, the counts
the definition of include/ext/tetra_biterr.h gives for those bits, and for the list rows the reference's bits and verdicts and the ranks
of include/ext/tetra_list.h's definition with eight candidates.

    python -m tests.golden.make_lmac_soft_golden
"""
import hashlib
import os

import numpy as np

from tests import list_definition as D
from tests import soft_pipeline as sp
from tests.golden import make_list_golden

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "lmac_soft_golden.npz")
KINDS = ("sb1", "sb2", "ndb1", "ndb2", "schf")


def planted(kind, encoder=sp.DefinitionEncoder):
    """The planted rows of a kind and their scrambling codes (tests/soft_pipeline.soft_rows_for, the seeds of tests/test_rx_soft.py)."""
    return sp.soft_rows_for(encoder, kind, np.random.default_rng(100 + KINDS.index(kind)))


def list_rows(kind):
    """The soft rows of tests/golden/list_golden.npz, whose case coverage tests/test_list_decode.py asserts, and their codes."""
    g = np.load(make_list_golden.PATH)
    return g["soft_%s_soft" % kind], g["soft_%s_si" % kind]


def checksum(rows, codes):
    h = hashlib.sha256(np.ascontiguousarray(rows, np.int8).tobytes() + np.ascontiguousarray(codes, np.uint32).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def decode_all(lref, t, rows, codes):
    got = [sp.ref_soft_decode(lref, t, r, int(c)) for r, c in zip(rows, codes)]
    return np.array([g[0] for g in got], np.uint8), np.array([g[1] for g in got], np.int32)


def counts_of(t, rows, codes, type2):
    """errors | compared << 16 per row, on the soft values, for the rows' decoded bits"""
    ec = [D.count_errors(t, r, int(c), d, soft=True) for r, c, d in zip(rows, codes, type2)]
    return np.array([e | (c << 16) for e, c in ec], np.uint32)


def make(lref):
    out = {}
    for kind in KINDS:
        t = sp.REF_TPSAP[kind]
        rows, codes = planted(kind)
        t2, ok = decode_all(lref, t, rows, codes)
        out[kind + "_sum"], out[kind + "_t2"], out[kind + "_ok"] = checksum(rows, codes), np.packbits(t2, axis=1), ok
        out[kind + "_biterr"] = counts_of(t, rows, codes, t2)
        rows, codes = list_rows(kind)
        t2, ok = decode_all(lref, t, rows, codes)
        out[kind + "_list_sum"], out[kind + "_list_t2"], out[kind + "_list_ok"] = checksum(rows, codes), np.packbits(t2, axis=1), ok
        out[kind + "_list_rank"] = D.list_decode(t, D.soft_values(t, rows, codes), 8, D.START_SOFT)["rank"]
    return out


if __name__ == "__main__":
    from oracle import ref_binding
    assert ref_binding.lmac_available(), "needs oracle/_ref/libtetra_lmac_ref.so"
    data = make(ref_binding)
    np.savez_compressed(PATH, **data)
    print(PATH, os.path.getsize(PATH), "bytes")
