"""Writes tests/golden/list_golden.npz: the damaged rows the list-decoding tests (tests/test_list_decode.py) run on, made with the
REFERENCE's encoder (oracle/_ref/libtetra_lmac_ref.so through oracle/ref_binding.lmac_encode) from fixed seeds, and the reference's own
decoding of each (lmac_decode / conv_cch_decode on soft values): the maximum-likelihood rows and verdicts the definition's ML path is held
against where the reference is not at hand.  Only inputs and the reference's outputs: no rank, no rescued row.

    python -m tests.golden.make_list_golden
"""
import os

import numpy as np

from tests import list_definition as D
from tests import soft_pipeline as sp

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "list_golden.npz")
CODED = (0, 1, 2, 4, 5)
RATE = {0: 0.045, 1: 0.04, 2: 0.04, 4: 0.04, 5: 0.033}           # flip rates at which about half of a kind's blocks fail
SOFT_KINDS = {"sb1": 0, "sb2": 1, "ndb1": 2, "ndb2": 2, "schf": 5}
SIGMA = {0: 0.74, 1: 0.70, 2: 0.70, 5: 0.64}
N_CLEAN, N_NOISY, N_ERASED, N_EDGE = 24, 96, 24, 16
PLACE = {(0, 1): [(94, 120)], (1, 2): [(282, 216)], (2, 1): [(14, 216)], (2, 2): [(282, 216)], (5, 0): [(14, 216), (282, 216)]}


def hard_pool(lref, t):
    """N_CLEAN clean rows, N_NOISY with random flips, N_ERASED with flips and a twentieth of the positions erased (0xff after
    descrambling), N_EDGE whose flips sit on the coded bits of the first (even rows) or the last (odd rows) six trellis steps."""
    rng = np.random.default_rng(7100 + t)
    n345, n2, n1, a = D.BLK[t]
    n = N_CLEAN + N_NOISY + N_ERASED + N_EDGE
    si = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if t == 0:
        si[:] = D.SCRAMB_INIT
    pos4 = (a * np.arange(1, n345 + 1)) % n345                   # type-4 position of type-3 bit j
    rows = np.zeros((n, n345), np.uint8)
    for b in range(n):
        row = lref.lmac_encode(t, rng.integers(0, 2, n1).astype(np.uint8), int(si[b]))
        if b >= N_CLEAN + N_NOISY + N_ERASED:
            k = b - (N_CLEAN + N_NOISY + N_ERASED)
            edge = np.arange(9) if k % 2 == 0 else np.arange(n345 - 9, n345)         # type-3 bits of six steps
            hit = rng.choice(edge, 3 + k // 6, replace=False)
            row[pos4[hit]] ^= 1
            row ^= (rng.random(n345) < 0.01).astype(np.uint8)
        elif b >= N_CLEAN:
            row ^= (rng.random(n345) < RATE[t]).astype(np.uint8)
        if N_CLEAN + N_NOISY <= b < N_CLEAN + N_NOISY + N_ERASED:
            pick = rng.random(n345) < 0.05
            row[pick] = 0xff ^ D.scramb_seq(int(si[b]), n345)[pick]
        rows[b] = row
    want = np.zeros((n, n2), np.uint8)
    ok = np.zeros(n, np.int32)
    for b in range(n):
        want[b], ok[b] = lref.lmac_decode(t, rows[b], si[b])
    return rows, si, want, ok


def soft_pool(lref, kind, t, n=64):
    """Encoded blocks as 6-bit soft values: +-16 plus Gaussian noise, rounded and clipped to +-31 (the chain's quantiser at G = 16)."""
    rng = np.random.default_rng(7200 + sorted(SOFT_KINDS).index(kind))
    n345, n2, n1, a = D.BLK[t]
    si = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if t == 0:
        si[:] = D.SCRAMB_INIT
    soft = np.zeros((n, n345), np.int8)
    want = np.zeros((n, n2), np.uint8)
    ok = np.zeros(n, np.int32)
    for b in range(n):
        bits = lref.lmac_encode(t, rng.integers(0, 2, n1).astype(np.uint8), int(si[b]))
        v = 16.0 * ((1.0 - 2.0 * bits) + SIGMA[t] * rng.standard_normal(n345))
        soft[b] = np.clip(np.rint(v), -31, 31)
        want[b], ok[b] = sp.ref_soft_decode(lref, t, soft[b], int(si[b]))
    return soft, si, want, ok


def frame_pool(lref, n=104):
    """n frames (512 bytes of bits each) of the three downlink burst types and a few that carry nothing; every block position holds an
    encoded block under the frame's scrambling code with random flips."""
    rng = np.random.default_rng(7300)
    types = rng.choice(np.array([0, 1, 3, 0, 1, 3, 2, -1], np.int32), n)
    codes = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    frames = np.zeros((n, 512), np.uint8)
    frames[:, :510] = rng.integers(0, 2, (n, 510))
    for r in range(n):
        for (tpsap, blk), pieces in PLACE.items():
            train = {0: 3, 1: 3, 2: 1, 5: 0}[tpsap]
            if types[r] != train:
                continue
            n345, _, n1, _ = D.BLK[tpsap]
            t5 = lref.lmac_encode(tpsap, rng.integers(0, 2, n1).astype(np.uint8), D.SCRAMB_INIT if tpsap == 0 else int(codes[r]))
            t5 = t5 ^ (rng.random(n345) < (0.0 if r % 4 == 0 else RATE[tpsap])).astype(np.uint8)
            at = 0
            for off, ln in pieces:
                frames[r, off:off + ln] = t5[at:at + ln]
                at += ln
    return frames, types, codes


def make(lref):
    out = {}
    for t in CODED:
        rows, si, want, ok = hard_pool(lref, t)
        out["hard%d_rows" % t], out["hard%d_si" % t], out["hard%d_want" % t], out["hard%d_ok" % t] = rows, si, want, ok
    for kind, t in SOFT_KINDS.items():
        soft, si, want, ok = soft_pool(lref, kind, t)
        out["soft_%s_soft" % kind], out["soft_%s_si" % kind], out["soft_%s_want" % kind], out["soft_%s_ok" % kind] = soft, si, want, ok
    frames, types, codes = frame_pool(lref)
    out["frames_bits"], out["frames_types"], out["frames_codes"] = np.packbits(frames, axis=1), types, codes
    return out


if __name__ == "__main__":
    from oracle import ref_binding
    assert ref_binding.lmac_available(), "needs oracle/_ref/libtetra_lmac_ref.so"
    data = make(ref_binding)
    np.savez_compressed(PATH, **data)
    print(PATH, os.path.getsize(PATH), "bytes")
