"""The circuit-mode data channels (include/ext/tetra_tch.h) as the reference's own functions define them: the exported primitives of
oracle/_ref/libtetra_lmac_ref.so chained in the order of tp_sap_udata_ind, the encoder chain as known-answer generator, the bit-error
definition, and the row sets the tests and the golden file (tests/golden/make_lmac_tch_golden.py) share."""
import ctypes as C
import os

import numpy as np

TCH_7_2, TCH_4_8, TCH_2_4 = 8, 9, 10
CODED = (TCH_4_8, TCH_2_4)
# kind -> (type345, type2, type1, interleave a); puncturer = enum tetra_rcpc_puncturer (lower_mac/tetra_conv_enc.h)
BLK = {TCH_7_2: (432, 432, 432, 0), TCH_4_8: (432, 292, 288, 103), TCH_2_4: (432, 148, 144, 103)}
PUNCT = {TCH_4_8: 2, TCH_2_4: 3}            # TETRA_RCPC_PUNCT_292_432, TETRA_RCPC_PUNCT_148_432
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lmac_tch_golden.npz")
N_RANDOM, N_CODED = 200, 64


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def descramble(L, row, code):
    """tetra_scramb_bits on the row's 432 bytes (XORs the sequence's bit onto every byte)."""
    t4 = np.ascontiguousarray(row, np.uint8)[:432].copy()
    L.tetra_scramb_bits(int(code) & 0xffffffff, _p(t4), 432)
    return t4


def decode(L, kind, row, code):
    """One row through the definition -> type2 bytes."""
    n345, n2, _, a = BLK[kind]
    t4 = descramble(L, row, code)
    if kind == TCH_7_2:
        return t4 & 1
    t3 = np.zeros(n345, np.uint8)
    L.block_deinterleave(n345, a, _p(t4), _p(t3))
    mother = np.full(4 * (n2 + 8), 0xff, np.uint8)
    L.tetra_rcpc_depunct(PUNCT[kind], _p(t3), n345, _p(mother))
    out = np.zeros(n2 + 8, np.uint8)
    L.viterbi_dec_sb1_wrapper(_p(mother), _p(out), n2)
    return out[:n2].copy()


def reencode(L, kind, type2):
    """The type-4 bits a transmitter would send for these type-2 bits (all of them, tail included), before scrambling."""
    n345, n2, _, a = BLK[kind]
    d = np.ascontiguousarray(type2, np.uint8)[:n2].copy()
    ces = np.zeros(64, np.uint8)
    L.conv_enc_init(_p(ces))
    mother = np.zeros(4 * n2, np.uint8)
    L.conv_enc_input(_p(ces), _p(d), n2, _p(mother))
    t3 = np.zeros(n345, np.uint8)
    L.get_punctured_rate(PUNCT[kind], _p(mother), n345, _p(t3))
    t4 = np.zeros(n345, np.uint8)
    L.block_interleave(n345, a, _p(t3), _p(t4))
    return t4


def encode(L, kind, type1, code):
    """type-1 payload -> type-5 bits (four zero tail bits appended)."""
    n345, n2, n1, _ = BLK[kind]
    d = np.zeros(n2, np.uint8)
    d[:n1] = np.asarray(type1, np.uint8)[:n1]
    t5 = reencode(L, kind, d)
    L.tetra_scramb_bits(int(code) & 0xffffffff, _p(t5), n345)
    return t5


def biterr_word(L, kind, row, code, type2):
    """errors | compared << 16 of include/ext/tetra_biterr.h for a received byte row and its decoded bits."""
    e = reencode(L, kind, type2)
    r = descramble(L, row, code)
    valid = r != 0xff
    errors = int((valid & ((r != 0) != (e != 0))).sum())
    return errors | (int(valid.sum()) << 16)


def depunct_patterns(L, kind):
    """The per-step patterns of the kind's puncturer, from tetra_rcpc_depunct of an all-zero row into 0xff bytes: uint8 [type2],
    g1 g2 g3 g4 at bits 3..0 (1 = the generator's bit is sent)."""
    n345, n2, _, _ = BLK[kind]
    mother = np.full(4 * (n2 + 8), 0xff, np.uint8)
    L.tetra_rcpc_depunct(PUNCT[kind], _p(np.zeros(n345, np.uint8)), n345, _p(mother))
    sent = (mother[:4 * n2] == 0).reshape(n2, 4).astype(np.uint8)
    assert (mother[4 * n2:] == 0xff).all()
    return sent[:, 0] << 3 | sent[:, 1] << 2 | sent[:, 2] << 1 | sent[:, 3]


def codes(rng, n):
    """scrambling codes 0 and 3 (SCRAMB_INIT) first, then random ones"""
    c = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    c[0], c[1] = 0, 3
    return c


def make_inputs(L):
    """The row sets, inputs only (fixed seeds).  bits / bytes: 200 rows each, shared by all three kinds; per coded kind 64 encoded blocks
    (clean) and the same with 1..40 flipped bits (noisy)."""
    rng = np.random.default_rng(20240)
    z = {}
    z["bits"] = rng.integers(0, 2, (N_RANDOM, 432)).astype(np.uint8)
    z["bits_code"] = codes(rng, N_RANDOM)
    # arbitrary bytes: 0, 1, 0xff and 2..254 mixed, in every row
    pick = rng.integers(0, 4, (N_RANDOM, 432))
    other = rng.integers(2, 255, (N_RANDOM, 432))
    z["bytes"] = np.where(pick == 0, 0, np.where(pick == 1, 1, np.where(pick == 2, 0xff, other))).astype(np.uint8)
    z["bytes_code"] = codes(rng, N_RANDOM)
    for kind in CODED:
        n1 = BLK[kind][2]
        pay = rng.integers(0, 2, (N_CODED, n1)).astype(np.uint8)
        code = codes(rng, N_CODED)
        clean = np.stack([encode(L, kind, pay[b], code[b]) for b in range(N_CODED)])
        noisy = clean.copy()
        flips = 1 + (np.arange(N_CODED) * 39) // (N_CODED - 1)          # 1 .. 40
        for b in range(N_CODED):
            noisy[b, rng.choice(432, int(flips[b]), replace=False)] ^= 1
        z["pay_%d" % kind], z["code_%d" % kind], z["clean_%d" % kind], z["noisy_%d" % kind] = pay, code, clean, noisy
    return z


def sets_of(z, kind):
    """(name, rows, codes) of every row set a kind is tested on"""
    s = [("bits", z["bits"], z["bits_code"]), ("bytes", z["bytes"], z["bytes_code"])]
    if kind in CODED:
        s += [("clean", z["clean_%d" % kind], z["code_%d" % kind]), ("noisy", z["noisy_%d" % kind], z["code_%d" % kind])]
    return s


def expected(L, z):
    """The reference's decoding of every row set of every kind, and the definition's bit-error words of the coded ones:
    want_<kind>_<set>, be_<kind>_<set>."""
    out = {}
    for kind in (TCH_7_2,) + CODED:
        for name, rows, code in sets_of(z, kind):
            want = np.stack([decode(L, kind, rows[b], code[b]) for b in range(len(rows))])
            out["want_%d_%s" % (kind, name)] = want
            if kind in CODED:
                out["be_%d_%s" % (kind, name)] = np.array([biterr_word(L, kind, rows[b], code[b], want[b]) for b in range(len(rows))], np.uint32)
    return out


def load_golden():
    with np.load(GOLDEN) as f:
        z = {k: f[k] for k in f.files}
    for k in ("bits",) + tuple("%s_%d" % (s, kind) for kind in CODED for s in ("clean", "noisy", "pay")):
        z[k] = np.unpackbits(z[k], axis=1)[:, :int(z[k + "_cols"])]         # plain-bit sets are stored packed
    for a in z.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return z
