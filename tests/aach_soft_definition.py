"""The soft AACH decoder's definition (include/ext/tetra_aach_soft.h) in numpy: exact maximum-likelihood decoding of the RM(30,14) code
over all 16384 codewords, chunked over blocks.  A helper for tests/test_aach_soft.py and the GPU tests, not a test; nothing of the
product's code runs here.  The codeword list is the recorded one of the reference's encoder (tests/golden/rm3014_codewords.npy, in
info order), so the definition does not lean on the code under test for the code either.

    corr(c) = sum y[i] (1 - 2 c[i]);  best = arg max, ties to the smallest info;  margin = (corr(best) - max over the others) / 2;
    dist = |{i: y[i] != 0, sign disagrees with best}|;  crc_ok = margin >= min_margin;  row = best's 30 bits, dist, min(margin, 255)
"""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
Q, G = 31, 16.0
MAX_MARGIN = 30 * Q


@functools.lru_cache(None)
def codewords():
    """uint32 [16384]: codeword of info = index, first bit on air at bit 29."""
    cw = np.load(os.path.join(HERE, "golden", "rm3014_codewords.npy")).astype(np.uint32)
    assert cw.shape == (16384,) and np.array_equal(cw >> 16, np.arange(16384))          # systematic, in info order
    return cw


@functools.lru_cache(None)
def code_bits():
    """uint8 [16384][30]: bit i of every codeword in air order."""
    return ((codewords()[:, None] >> (29 - np.arange(30))[None, :]) & 1).astype(np.uint8)


@functools.lru_cache(None)
def _signs():
    return np.ascontiguousarray((1 - 2 * code_bits().astype(np.float32)).T)          # [30][16384]; float32 holds |corr| <= 930 exactly


def decode(soft, chunk=512):
    """soft: int [n][>= 30] (the first 30 of a row used, |y| <= 31) -> (info int64 [n], margin int64 [n], dist int64 [n])."""
    y = np.asarray(soft)[:, :30].astype(np.int64)
    assert np.abs(y).max(initial=0) <= Q
    n = len(y)
    info, margin, dist = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    bits = code_bits()
    for a in range(0, n, chunk):
        yc = y[a:a + chunk]
        corr = np.rint(yc.astype(np.float32) @ _signs()).astype(np.int64)          # [rows][16384]
        best = corr.argmax(axis=1)                                                 # (the first maximum: the smallest info)
        top = corr[np.arange(len(yc)), best]
        corr[np.arange(len(yc)), best] = -(1 << 20)
        diff = top - corr.max(axis=1)
        assert np.all(diff >= 0) and np.all(diff % 2 == 0)
        info[a:a + chunk], margin[a:a + chunk] = best, diff // 2
        dist[a:a + chunk] = ((yc != 0) & ((yc < 0) != (bits[best] != 0))).sum(axis=1)
    return info, margin, dist


def rows(soft, min_margin=1):
    """-> (rows uint8 [n][32], crc_ok int32 [n]): the row format and the verdict."""
    info, margin, dist = decode(soft)
    out = np.zeros((len(info), 32), np.uint8)
    out[:, :30] = code_bits()[info]
    out[:, 30] = dist
    out[:, 31] = np.minimum(margin, 255)
    return out, (margin >= max(1, int(min_margin))).astype(np.int32)


def descramble(soft30, seq_bits):
    """30 ring values and the scrambling sequence's 30 bits -> the block's values (negated where the sequence has a 1)."""
    v = np.asarray(soft30).astype(np.int64)
    return np.where(np.asarray(seq_bits) != 0, -v, v)


def toy_rows(rng, n, sigma):
    """The toy channel of the issue: random codewords sent as +-1, Gaussian noise of `sigma`, quantised with G = 16, Q = 31
    -> (int8 [n][32], the sent info)."""
    info = rng.integers(0, 16384, n)
    tx = 1.0 - 2.0 * code_bits()[info]
    q = np.clip(np.rint(G * (tx + rng.normal(0, sigma, tx.shape))), -Q, Q)
    out = np.zeros((n, 32), np.int8)
    out[:, :30] = q
    return out, info
