"""An independent statement of the CRC-aided list decoding of include/ext/tetra_list.h in numpy: a plain 16-state Viterbi decoder over
the K = 5 mother code with the rate-2/3 puncturing, which stores every decision and every add-compare-select difference, and from them
the margins, the candidate order, the candidate tracebacks and the CRC.  Nothing of the product is used: the scrambler, the interleaver,
the generators and the CRC are written out here from EN 300 392-2 (8.2.3.1.1, 8.2.4, 8.2.5) and ITU-T X.25's CRC16."""
import numpy as np

# type345, type2, type1, interleaver a, by TPSAP type (SB1, SB2, NDB, -, SCH/HU, SCH/F)
BLK = {0: (120, 80, 60, 11), 1: (216, 144, 124, 101), 2: (216, 144, 124, 101), 4: (168, 112, 92, 13), 5: (432, 288, 268, 103)}
SCRAMB_INIT = 3
TAPS = (32, 26, 23, 22, 16, 12, 11, 10, 8, 7, 5, 4, 2, 1)
START_HARD, START_SOFT = 20, 2540                # 127 * 4 * 5 in units of 127, and raw


def scramb_seq(code, n):
    """The scrambling sequence of a 32-bit code: a Fibonacci LFSR that shifts right, the new bit entering at bit 31."""
    lfsr, out = int(code) & 0xffffffff, np.zeros(n, np.uint8)
    for i in range(n):
        bit = 0
        for y in TAPS:
            bit ^= (lfsr >> (32 - y)) & 1
        lfsr = (lfsr >> 1) | (bit << 31)
        out[i] = bit
    return out


def type3_values(t, values4):
    """[rows][type345] descrambled values in type-4 order -> type-3 order: type3[i - 1] = type4[(a i) % K], i = 1 .. K."""
    n345, _, _, a = BLK[t]
    return values4[:, (a * np.arange(1, n345 + 1)) % n345]


def hard_values(t, rows, codes):
    """Byte rows (still scrambled) -> [rows][type345] values in type-3 order in units of 127: a descrambled 0 is +1, 0xff an erasure
    (0), anything else -1."""
    n345 = BLK[t][0]
    v = np.zeros((len(rows), n345), np.int64)
    for b in range(len(rows)):
        d = np.asarray(rows[b][:n345], np.uint8) ^ scramb_seq(SCRAMB_INIT if t == 0 else codes[b], n345)
        v[b] = np.where(d == 0, 1, np.where(d == 0xff, 0, -1))
    return type3_values(t, v)


def soft_values(t, soft5, codes):
    """Soft values as received (int8, positive = 0, still scrambled) -> type-3 order, descrambled by sign."""
    n345 = BLK[t][0]
    v = np.zeros((len(soft5), n345), np.int64)
    for b in range(len(soft5)):
        seq = scramb_seq(SCRAMB_INIT if t == 0 else codes[b], n345)
        v[b] = np.where(seq != 0, -np.asarray(soft5[b][:n345], np.int64), np.asarray(soft5[b][:n345], np.int64))
    return type3_values(t, v)


def crc_good(bits):
    """CRC16-CCITT (x^16 + x^12 + x^5 + 1) over [rows][n] bits, start 0xffff, good residue 0x1d0f."""
    r = np.full(len(bits), 0xffff, np.int64)
    for i in range(bits.shape[1]):
        fb = ((r >> 15) & 1) ^ bits[:, i]
        r = ((r << 1) & 0xffff) ^ (fb * 0x1021)
    return r == 0x1d0f


def list_decode(t, v3, T, start, forced_first=None):
    """v3 [rows][type345] values in type-3 order; start = the start metric of state 0.  Returns a dict: ml [rows][type2] and ml_ok (the
    decoder's result), out / ok / rank (after the rescue with T candidates), order [rows][8] (the steps of the first eight candidates),
    delta [rows][N] (every step's margin), win_step (the winner's step, -1).  forced_first: also return first_bits [rows][N], the
    traceback with the decision of that step inverted on every row."""
    n345, n2, n1, _ = BLK[t]
    rows, N = len(v3), n2 + 4
    # per step the two transmitted generator values (g1, g2); rate 2/3: type-3 bit 3u -> g1 of step 2u, 3u+1 -> g2 of step 2u,
    # 3u+2 -> g1 of step 2u+1; everything else (g2 of odd steps, g3, g4, the flush steps) is punctured or zero
    s1, s2 = np.zeros((rows, N), np.int64), np.zeros((rows, N), np.int64)
    s1[:, 0:n2:2], s2[:, 0:n2:2], s1[:, 1:n2:2] = v3[:, 0::3], v3[:, 1::3], v3[:, 2::3]
    # state = the four newest input bits, newest at bit 3; new state n comes from p0 = (2n) & 15 (even) or p0 + 1 with input n >> 3
    st = np.arange(16)
    p0, p1, inp = (2 * st) & 15, ((2 * st) & 15) | 1, st >> 3

    def gens(p):        # d1 = bit 3 of p (the previous input) .. d4 = bit 0; g1 = 1 + D + D^4, g2 = 1 + D^2 + D^3 + D^4
        d1, d2, d3, d4 = (p >> 3) & 1, (p >> 2) & 1, (p >> 1) & 1, p & 1
        return inp ^ d1 ^ d4, inp ^ d2 ^ d3 ^ d4

    g1e, g2e = gens(p0)
    g1o, g2o = gens(p1)
    M = np.zeros((rows, 16), np.int64)
    M[:, 0] = start
    dec = np.zeros((rows, N, 16), np.uint8)
    diff = np.zeros((rows, N, 16), np.int64)
    for k in range(N):
        a, b = s1[:, k, None], s2[:, k, None]
        even = M[:, p0] + a * (1 - 2 * g1e) + b * (1 - 2 * g2e)
        odd = M[:, p1] + a * (1 - 2 * g1o) + b * (1 - 2 * g2o)
        diff[:, k] = even - odd
        dec[:, k] = even < odd                  # ties keep the even predecessor
        M = np.maximum(even, odd)
    assert np.abs(diff).max() < 32768

    def trace(flip):        # flip [rows]: the step whose decision is inverted (-1: none) -> bits [rows][N], states after each step
        s = np.zeros(rows, np.int64)
        bits, states = np.zeros((rows, N), np.uint8), np.zeros((rows, N), np.int64)
        r = np.arange(rows)
        for k in range(N - 1, -1, -1):
            states[:, k] = s
            bits[:, k] = s >> 3
            d = dec[r, k, s] ^ (flip == k)
            s = ((2 * s) & 15) | d
        return bits, states

    ml_bits, ml_states = trace(np.full(rows, -1))
    ml = ml_bits[:, :n2]
    ml_ok = crc_good(ml[:, :n1 + 16])
    r = np.arange(rows)
    delta = np.abs(diff[r[:, None], np.arange(N)[None, :], ml_states])
    order = np.argsort(delta * 1024 + np.arange(N)[None, :], axis=1, kind="stable")[:, :8]
    out, ok, rank, win = ml.copy(), ml_ok.copy(), np.where(ml_ok, 0, -1), np.full(rows, -1)
    for k in range(T):
        todo = ~ok
        if not todo.any():
            break
        bits, _ = trace(np.where(todo, order[:, k], -1))
        good = crc_good(bits[:, :n1 + 16]) & todo
        out[good], rank[good], win[good] = bits[good, :n2], k + 1, order[good, k]
        ok |= good
    res = dict(ml=ml, ml_ok=ml_ok.astype(np.int32), out=out, ok=ok.astype(np.int32), rank=rank.astype(np.int32), order=order, delta=delta,
               win_step=win)
    if forced_first is not None:
        res["first_bits"] = trace(np.full(rows, forced_first))[0]
    return res


def type4_of(t, type2):
    """Type-2 bits (tail included) encoded from the all-zero state (g1, g2 of every even step, g1 of every odd one) and interleaved."""
    n345, n2, _, a = BLK[t]
    d = np.concatenate([np.zeros(4, np.int64), np.asarray(type2[:n2], np.int64)])
    k = np.arange(n2) + 4
    g1 = d[k] ^ d[k - 1] ^ d[k - 4]
    g2 = d[k] ^ d[k - 2] ^ d[k - 3] ^ d[k - 4]
    type3 = np.zeros(n345, np.int64)
    type3[0::3], type3[1::3], type3[2::3] = g1[0::2], g2[0::2], g1[1::2]
    type4 = np.zeros(n345, np.int64)
    type4[(a * np.arange(1, n345 + 1)) % n345] = type3
    return type4


def encode(t, type1, code):
    """A transmitter: type-1 bits -> type-5 bits uint8 [type345].  The CRC appended is the ones' complement of crc_good's register over
    the type-1 bits, first bit most significant; then four zero tail bits, type4_of, and the scrambling sequence of the block's code."""
    n345, n2, n1, _ = BLK[t]
    r = 0xffff
    for b in np.asarray(type1[:n1], np.int64):
        r = ((r << 1) & 0xffff) ^ ((((r >> 15) & 1) ^ int(b)) * 0x1021)
    type2 = np.zeros(n2, np.int64)
    type2[:n1] = type1[:n1]
    type2[n1:n1 + 16] = [((r ^ 0xffff) >> (15 - i)) & 1 for i in range(16)]
    assert crc_good(type2[None, :n1 + 16])[0]
    return (type4_of(t, type2) ^ scramb_seq(SCRAMB_INIT if t == 0 else code, n345)).astype(np.uint8)


def count_errors(t, row, code, type2, soft=False):
    """(errors, compared) of include/ext/tetra_biterr.h for a received byte row and decoded type-2 bits: the bits encoded again from the
    all-zero state (g1, g2 of every even step, g1 of every odd one), interleaved, and held against the descrambled row where it is
    not an erasure."""
    n345 = BLK[t][0]
    type4 = type4_of(t, type2)
    seq = scramb_seq(SCRAMB_INIT if t == 0 else code, n345)
    if soft:        # soft values as received (positive = 0): zero carries no decision, negative after descrambling is a 1
        v = np.where(seq != 0, -np.asarray(row[:n345], np.int64), np.asarray(row[:n345], np.int64))
        valid = v != 0
        return int((valid & ((v < 0) != (type4 != 0))).sum()), int(valid.sum())
    desc = np.asarray(row[:n345], np.uint8) ^ seq
    valid = desc != 0xff
    return int((valid & ((desc != 0) != (type4 != 0))).sum()), int(valid.sum())
