"""TCH/4.8 and TCH/2.4 from soft values (include/ext/tetra_tch_soft.h) as the reference's own functions define them: the signalling
kinds' soft chain (tests/soft_pipeline.ref_soft_decode) with the TCH puncturers of tests/tch_definition.py, the definition of the
channel bit-error count on soft values, and the row sets that the tests and the fixture (tests/golden/make_lmac_tch_soft_golden.py) share.
Nothing of the product's code runs here."""
import ctypes as C
import os

import numpy as np

from tests import tch_definition as td

TCH_4_8, TCH_2_4 = td.TCH_4_8, td.TCH_2_4
CODED = td.CODED
BLK = td.BLK
Q = 31                                   # csrc/soft_core.hpp kQ
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lmac_tch_soft_golden.npz")
SIGMA = {TCH_4_8: 8.0, TCH_2_4: 16.0}    # of the noisy set that is held against the hard definition
N_NOISY = 64
FIXED_CODES = (0, 3, 0xffffffff)
# the sets in order, with their sizes; `gain` is the noisy set at amplitude 16 and SIGMA[kind]
SETS = (("clean", 16), ("gain", N_NOISY), ("noisy", 12), ("random", 24), ("bound", 16), ("zero", 4), ("sparse", 8))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def sequence(L, code):
    seq = np.zeros(432, np.uint8)
    L.tetra_scramb_bits(int(code) & 0xffffffff, _p(seq), 432)
    return seq


def descramble(L, soft5, code):
    """type-5 soft values -> type-4: negated where the scrambling sequence has a 1"""
    v = np.ascontiguousarray(soft5, np.int8)[:432]
    return np.where(sequence(L, code) != 0, -v, v).astype(np.int8)


def decode(L, kind, soft5, code):
    """One block of 432 int8 soft values through the definition -> type2 bytes."""
    L.conv_cch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    n345, n2, _, a = BLK[kind]
    t4 = descramble(L, soft5, code)
    t3 = np.zeros(n345, np.int8)
    L.block_deinterleave(n345, a, _p(t4), _p(t3))
    mother = np.zeros(4 * (n2 + 8), np.int8)                # punctured positions: 0
    L.tetra_rcpc_depunct(td.PUNCT[kind], _p(t3), n345, _p(mother))
    out = np.zeros(n2 + 8, np.uint8)
    L.conv_cch_decode(_p(mother), _p(out), n2)
    return out[:n2].copy()


def biterr_word(L, kind, soft5, code, type2):
    """errors | compared << 16: the positions whose descrambled value is not 0 are compared, an error is a sign that differs from the
    re-encoded bit"""
    e = td.reencode(L, kind, type2)
    r = descramble(L, soft5, code).astype(np.int32)
    valid = r != 0
    return int((valid & ((r < 0) != (e != 0))).sum()) | (int(valid.sum()) << 16)


def hard_rows(soft):
    """the hard decisions of soft rows as byte rows of tests/tch_definition.py: the signs (a zero counts as bit 0)"""
    return (np.asarray(soft) < 0).astype(np.uint8)


def make_inputs(L):
    """The row sets of both coded kinds, inputs only (fixed seed): soft_<kind> int8 [144][432] and code_<kind> uint32 [144] in the order
    of SETS, pay_<kind> uint8 [16 + 64 + 12][type1] the payloads of the clean, gain and noisy rows."""
    rng = np.random.default_rng(4824)
    z = {}
    for kind in CODED:
        n1 = BLK[kind][2]
        rows, codes, pays = [], [], []

        def codeword(code):
            pay = rng.integers(0, 2, n1).astype(np.uint8)
            pays.append(pay)
            return 1 - 2 * td.encode(L, kind, pay, code).astype(np.int32)

        def some_code():
            return int(rng.integers(0, 1 << 32))
        for i in range(16):                                  # clean, four at each amplitude
            code = (FIXED_CODES + (some_code(),))[i % 4] if i < 4 else some_code()
            rows.append(codeword(code) * (Q, 16, 5, 1)[i // 4]), codes.append(code)
        for i in range(N_NOISY):
            code = some_code()
            rows.append(np.clip(np.rint(codeword(code) * 16 + rng.normal(0, SIGMA[kind], 432)), -Q, Q)), codes.append(code)
        for i in range(12):
            code = some_code()
            rows.append(np.clip(np.rint(codeword(code) * 16 + rng.normal(0, (4.0, 12.0, 24.0)[i % 3], 432)), -Q, Q)), codes.append(code)
        for i in range(24):
            rows.append(rng.integers(-Q, Q + 1, 432)), codes.append(some_code())
        alt = np.where(np.arange(432) % 2 == 0, Q, -Q)
        for r in (np.full(432, Q), np.full(432, -Q), alt, -alt, np.zeros(432)):          # the bound's rows, then the all-zero row
            for code in FIXED_CODES + (some_code(),):
                rows.append(r), codes.append(code)
        for i in range(8):                                   # mostly ties
            r = np.zeros(432)
            r[rng.integers(0, 432, 6)] = rng.integers(-Q, Q + 1, 6)
            rows.append(r), codes.append(some_code())
        z["soft_%d" % kind] = np.array(rows, np.int8)
        z["code_%d" % kind] = np.array(codes, np.uint32)
        z["pay_%d" % kind] = np.array(pays, np.uint8)
        assert len(rows) == sum(n for _, n in SETS) and len(pays) == 16 + N_NOISY + 12
    return z


def set_slice(name):
    at = 0
    for s, n in SETS:
        if s == name:
            return slice(at, at + n)
        at += n
    raise KeyError(name)


def expected(L, z):
    """want_<kind> uint8 [144][type2] and be_<kind> uint32 [144]: the definition on every row; hard_<kind> uint8 [64][type2]: the hard
    definition (tests/tch_definition.decode) on the signs of the gain set."""
    out = {}
    for kind in CODED:
        rows, code = z["soft_%d" % kind], z["code_%d" % kind]
        want = np.stack([decode(L, kind, rows[b], code[b]) for b in range(len(rows))])
        out["want_%d" % kind] = want
        out["be_%d" % kind] = np.array([biterr_word(L, kind, rows[b], code[b], want[b]) for b in range(len(rows))], np.uint32)
        g = set_slice("gain")
        out["hard_%d" % kind] = np.stack([td.decode(L, kind, hard_rows(r), c) for r, c in zip(rows[g], code[g])])
    return out


def load_golden():
    with np.load(GOLDEN) as f:
        z = {k: f[k] for k in f.files}
    for kind in CODED:
        for k in ("want_%d" % kind, "hard_%d" % kind, "pay_%d" % kind):        # plain-bit arrays are stored packed
            z[k] = np.unpackbits(z[k], axis=1)[:, :int(z[k + "_cols"])]
    for a in z.values():
        a.flags.writeable = False
    return z


def frames_pick():
    """The 100 rows of a kind that the frame tests plant, a frame each: every set whole but the gain set, of which the first 20."""
    g = set_slice("gain")
    return np.array([i for i in range(sum(n for _, n in SETS)) if not g.start + 20 <= i < g.stop])
