"""TCH/4.8 and TCH/2.4 interleaved over N blocks (include/ext/tetra_tch_nblk.h) as the clause and the reference's own functions define
them.  The receiver: a numpy gather by the header's formula between the reference's exported descrambler and its puncturer + decoder
(the chains of tests/tch_definition.py and tests/tch_soft_definition.py).  The transmitter: the diagonal interleaver of EN 300 392-2
8.2.4.2 looped over (m, k) as the standard writes it, independently of the gather, so that the known-answer tests hold one direction
against the other.  The count definition, and the input sets that the tests and the fixture (tests/golden/make_lmac_tch_nblk_golden.py)
share.  Nothing of the product's code runs here."""
import ctypes as C
import os

import numpy as np

from tests import tch_definition as td
from tests import tch_soft_definition as sd

TCH_4_8, TCH_2_4 = td.TCH_4_8, td.TCH_2_4
CODED = td.CODED
BLK = td.BLK
NS = (4, 8)
Q = sd.Q
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lmac_tch_nblk_golden.npz")
STREAM_BLOCKS = (12, 10, 8)              # payload blocks of the three streams
N_ARBITRARY = 16
INT32_MIN = -2 ** 31
AMPLITUDE = 16


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the receiver ---------------------------------------------------------------------------------------------------------------------
def type3_of(L, pool, codes, window, n_rows, soft):
    """The type-3 block of one window: type3[p] = the descrambled value of received row w[p mod N] at type-4 position
    (103 (j P + i + 1)) mod 432; a window entry outside [0, n_rows) is a lost row: 0xff (hard) or 0 (soft) throughout."""
    n = len(window)
    P = 432 // n
    t3 = np.full(432, 0 if soft else 0xff, np.int8 if soft else np.uint8)
    for j, r in enumerate(window):
        r = int(r)
        if not 0 <= r < n_rows:
            continue
        t4 = sd.descramble(L, pool[r], codes[r]) if soft else td.descramble(L, pool[r], codes[r])
        t3[j::n] = t4[(103 * (j * P + np.arange(P) + 1)) % 432]
    return t3


def decode_type3(L, kind, t3, soft):
    """type-3 block -> type2 bytes: the kind's depuncturer onto 0xff / zeros, then viterbi_dec_sb1_wrapper / conv_cch_decode."""
    n345, n2 = BLK[kind][0], BLK[kind][1]
    t3 = np.ascontiguousarray(t3)
    out = np.zeros(n2 + 8, np.uint8)
    if soft:
        L.conv_cch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        mother = np.zeros(4 * (n2 + 8), np.int8)
        L.tetra_rcpc_depunct(td.PUNCT[kind], _p(t3), n345, _p(mother))
        L.conv_cch_decode(_p(mother), _p(out), n2)
    else:
        mother = np.full(4 * (n2 + 8), 0xff, np.uint8)
        L.tetra_rcpc_depunct(td.PUNCT[kind], _p(t3), n345, _p(mother))
        L.viterbi_dec_sb1_wrapper(_p(mother), _p(out), n2)
    return out[:n2].copy()


def encode_type3(L, kind, type2):
    """type-2 bits (all of them, tail included) -> the 432 type-3 bits: mother code, then the kind's puncturer."""
    n345, n2 = BLK[kind][0], BLK[kind][1]
    d = np.ascontiguousarray(type2, np.uint8)[:n2].copy()
    ces = np.zeros(64, np.uint8)
    L.conv_enc_init(_p(ces))
    mother = np.zeros(4 * n2, np.uint8)
    L.conv_enc_input(_p(ces), _p(d), n2, _p(mother))
    t3 = np.zeros(n345, np.uint8)
    L.get_punctured_rate(td.PUNCT[kind], _p(mother), n345, _p(t3))
    return t3


def biterr_word(L, kind, t3, type2, soft):
    """errors | compared << 16 in the type-3 domain: the positions that are no erasure are compared, an error is a bit / sign that differs
    from the re-encoded bit"""
    e = encode_type3(L, kind, type2)
    r = np.asarray(t3).astype(np.int32)
    valid, one = (r != 0, r < 0) if soft else (r != 0xff, r != 0)
    return int((valid & (one != (e != 0))).sum()) | (int(valid.sum()) << 16)


def decode(L, kind, pool, codes, window, soft, n_rows=None):
    """One window through the definition -> (type2 bytes, count word)."""
    t3 = type3_of(L, pool, codes, window, len(pool) if n_rows is None else n_rows, soft)
    t2 = decode_type3(L, kind, t3, soft)
    return t2, biterr_word(L, kind, t3, t2, soft)


# ---- the transmitter, from the clause -------------------------------------------------------------------------------------------------
def diagonal_interleave(blocks3, n):
    """B3(1..M) -> B'3(1..M + N - 1):  b'3(m, k) = b3(m - j, j + 1 + i N) for 1 <= m - j <= M, else 0, with j = (k - 1) div (432 / N),
    i = (k - 1) mod (432 / N), k = 1 .. 432."""
    b3 = np.asarray(blocks3, np.uint8)
    M = len(b3)
    out = np.zeros((M + n - 1, 432), np.uint8)
    for m in range(1, M + n):
        for k in range(1, 433):
            j, i = (k - 1) // (432 // n), (k - 1) % (432 // n)
            if 1 <= m - j <= M:
                out[m - 1, k - 1] = b3[m - j - 1, j + i * n]           # b3(m - j, j + 1 + i N), 1-based
    return out


def transmit(L, kind, pays, n, code):
    """type-1 payloads [M][type1] of one stream -> its M + N - 1 bursts as type-5 bits: tail, mother code, puncturer, the diagonal
    interleaver, the (432, 103) block interleaver, the scrambler."""
    n2, n1 = BLK[kind][1], BLK[kind][2]
    b3 = []
    for pay in pays:
        d = np.zeros(n2, np.uint8)
        d[:n1] = pay
        b3.append(encode_type3(L, kind, d))
    rows = []
    for t3 in diagonal_interleave(b3, n):
        t3 = np.ascontiguousarray(t3)
        t5 = np.zeros(432, np.uint8)
        L.block_interleave(432, 103, _p(t3), _p(t5))
        L.tetra_scramb_bits(int(code) & 0xffffffff, _p(t5), 432)
        rows.append(t5)
    return np.array(rows, np.uint8)


# ---- the input sets -------------------------------------------------------------------------------------------------------------------
def sliding(at, length, n):
    """the windows of a stream of `length` received rows that starts at pool row `at`"""
    return [list(range(at + b, at + b + n)) for b in range(length - n + 1)]


def layout(n):
    """Where everything lies for interleaving depth n: the pool's row ranges and the window table's sets, as (name, windows) in order.
    Pool: the three clean streams, their noisy copies, the arbitrary rows.  The first 64 windows name plain-bit rows only, complete."""
    lengths = [m + n - 1 for m in STREAM_BLOCKS]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    per = int(starts[-1])
    arb = 2 * per
    n_rows = arb + N_ARBITRARY
    clean = [w for s in range(3) for w in sliding(int(starts[s]), lengths[s], n)]
    noisy = [[r + per for r in w] for w in clean]
    a = list(range(arb, n_rows))
    # plain rows, odd windows: a row n times (twice), rows of n different streams / codes (twice)
    across = [int(starts[(j % 3)]) + (j // 3) + 1 + (per if j % 2 else 0) for j in range(n)]
    odd_plain = [[3] * n, [per + int(starts[1]) + 2] * n, across, across[::-1]]
    arbitrary = sliding(arb, N_ARBITRARY, n)
    base, hurt = clean[2], noisy[STREAM_BLOCKS[0] + 3]
    lost = [[-1 if k == j else r for k, r in enumerate(base)] for j in range(n)] + [[-1 if k == j else r for k, r in enumerate(hurt)] for j in range(n)]
    all_lost = [[-1] * n]
    out_of_range = [[v if k == 1 else r for k, r in enumerate(base)] for v in (n_rows, n_rows + 5, -7, INT32_MIN)]
    odd_any = [[a[5]] * n, [a[(7 * j) % N_ARBITRARY] for j in range(n)]]
    # the third clean stream again with one burst lost, the one that N of its windows name: every window that names it says -1
    gone = int(starts[2]) + n - 1
    burst_lost = [[-1 if r == gone else r for r in w] for w in sliding(int(starts[2]), lengths[2], n)]
    sets = [("clean", clean), ("noisy", noisy), ("odd_plain", odd_plain), ("arbitrary", arbitrary), ("lost", lost), ("all_lost", all_lost),
            ("out_of_range", out_of_range), ("odd_any", odd_any), ("burst_lost", burst_lost)]
    return dict(n_rows=n_rows, starts=starts, lengths=lengths, per=per, arb=arb, sets=sets, gone=gone)


def windows_of(n):
    """The whole table: every set in order, then the same windows once more in shuffled order -> (int32 [n_blocks][n], slices by name)."""
    lay = layout(n)
    rows, where, at = [], {}, 0
    for name, w in lay["sets"]:
        where[name] = slice(at, at + len(w))
        rows += w
        at += len(w)
    first = np.array(rows, np.int64)
    order = np.random.default_rng(8240 + n).permutation(len(first))
    where["shuffled"] = slice(at, 2 * at)
    where["order"] = order
    return np.concatenate([first, first[order]]).astype(np.int32), where


def windows_n1(n_rows):
    """the short N = 1 table over the pool of depth 4: 20 rows spread over the pool, the last arbitrary rows, a lost one"""
    return np.array([[r] for r in list(range(0, n_rows - N_ARBITRARY, (n_rows - N_ARBITRARY) // 20))[:20] + list(range(n_rows - 6, n_rows)) + [-1, n_rows]],
                    np.int32)


def make_inputs(L):
    """Per coded kind and depth n (fixed seed): hard_<kind>_<n> uint8 / soft_<kind>_<n> int8 [n_rows][432], the pools; table_<kind>_<n>
    uint32, the distinct scrambling codes, and index_<kind>_<n> int32 [n_rows], each pool row's entry of it; pay_<kind>_<n> uint8
    [30][type1], the streams' payloads; win_<kind>_<n> int32, the window table; win_<kind>_1, the N = 1 table over the pools of depth 4."""
    z = {}
    for kind in CODED:
        n1 = BLK[kind][2]
        for n in NS:
            rng = np.random.default_rng(100 * kind + n)
            lay = layout(n)
            n_rows, per, arb = lay["n_rows"], lay["per"], lay["arb"]
            stream_code = np.array([0, 3, int(rng.integers(0, 1 << 32))], np.uint32)
            table = np.concatenate([stream_code, rng.integers(0, 1 << 32, N_ARBITRARY, dtype=np.uint64).astype(np.uint32)])
            index = np.zeros(n_rows, np.int32)
            hard = np.zeros((n_rows, 432), np.uint8)
            soft = np.zeros((n_rows, 432), np.int8)
            pays = []
            for s, m in enumerate(STREAM_BLOCKS):
                pay = rng.integers(0, 2, (m, n1)).astype(np.uint8)
                pays.append(pay)
                rows = transmit(L, kind, pay, n, stream_code[s])
                a, b = int(lay["starts"][s]), int(lay["starts"][s + 1])
                index[a:b] = index[per + a:per + b] = s
                hard[a:b] = rows
                soft[a:b] = AMPLITUDE * (1 - 2 * rows.astype(np.int32))
                flipped = rows.copy()
                for k in range(len(rows)):
                    flipped[k, rng.choice(432, int(rng.integers(1, 30)), replace=False)] ^= 1
                hard[per + a:per + b] = flipped
                soft[per + a:per + b] = np.clip(np.rint(AMPLITUDE * (1 - 2 * rows.astype(np.int32)) + rng.normal(0, sd.SIGMA[kind], rows.shape)), -Q, Q)
            index[arb:] = 3 + np.arange(N_ARBITRARY)
            pick = rng.integers(0, 4, (N_ARBITRARY, 432))
            other = rng.integers(2, 255, (N_ARBITRARY, 432))
            hard[arb:] = np.where(pick == 0, 0, np.where(pick == 1, 1, np.where(pick == 2, 0xff, other)))
            soft[arb:] = rng.integers(-Q, Q + 1, (N_ARBITRARY, 432))
            alt = np.where(np.arange(432) % 2 == 0, Q, -Q)
            soft[arb + 12:] = [np.full(432, Q), np.full(432, -Q), alt, np.zeros(432)]
            tag = "%d_%d" % (kind, n)
            z["hard_" + tag], z["soft_" + tag], z["table_" + tag], z["index_" + tag] = hard, soft, table, index
            z["pay_" + tag] = np.concatenate(pays)
            z["win_" + tag] = windows_of(n)[0]
        z["win_%d_1" % kind] = windows_n1(layout(4)["n_rows"])
    return z


def cases(kind):
    """(n, pool tag) of every window table of a kind: depth 1 runs over the pools of depth 4"""
    return [(1, "%d_4" % kind)] + [(n, "%d_%d" % (kind, n)) for n in NS]


def expected(L, z):
    """want_<mode>_<kind>_<n> uint8 [n_blocks][type2] and be_<mode>_<kind>_<n> uint32 [n_blocks], mode hard / soft: the definition on every
    window of every table."""
    out = {}
    for kind in CODED:
        for n, tag in cases(kind):
            codes = z["table_" + tag][z["index_" + tag]]
            win = z["win_%d_%d" % (kind, n)]
            for mode in ("hard", "soft"):
                pool = z[mode + "_" + tag]
                memo, t2s, bes = {}, [], []
                for w in win:
                    key = tuple(int(r) if 0 <= r < len(pool) else -1 for r in w)
                    if key not in memo:
                        memo[key] = decode(L, kind, pool, codes, w, mode == "soft")
                    t2s.append(memo[key][0]), bes.append(memo[key][1])
                out["want_%s_%d_%d" % (mode, kind, n)] = np.array(t2s, np.uint8)
                out["be_%s_%d_%d" % (mode, kind, n)] = np.array(bes, np.uint32)
    return out


PACKED = tuple("%s_%d_%d" % (k, kind, n) for kind in CODED for n in (1,) + NS for k in ("want_hard", "want_soft")) + \
    tuple("pay_%d_%d" % (kind, n) for kind in CODED for n in NS)


def load_golden():
    with np.load(GOLDEN) as f:
        z = {k: f[k] for k in f.files}
    for k in PACKED:                                           # plain-bit arrays are stored packed
        z[k] = np.unpackbits(z[k], axis=1)[:, :int(z[k + "_cols"])]
    for a in z.values():
        a.flags.writeable = False
    return z
