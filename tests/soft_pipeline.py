"""The receive chain's soft-decision option (TETRA_RX_FLAG_SOFT) restated on the host from the reference's own programs, for
tests/test_rx_soft.py: oracle symbols -> quantiser (numpy float32) -> the reference's soft decoder, and oracle bits -> the reference's
hard decoder, under the reference's clock and scrambling codes.  Nothing of the product's code runs here.

    soft decode of a block:  sign-descramble (tetra_scramb_bits on zeros gives the sequence) -> block_deinterleave -> tetra_rcpc_depunct
                             onto zeros -> conv_cch_decode (viterbi_cch.c -> osmo_conv.c) -> crc16_ccitt_bits
    hard decode:             ref_binding.lmac_decode (tp_sap_udata_ind's order of the same primitives)
"""
import ctypes as C

import numpy as np

from tests import chain_host as ch
from tests import list_definition

Q, G = 31, np.float32(16.0)                     # csrc/soft_core.hpp
FRESH_PREV = np.complex64(complex(np.float32(0.70710678), np.float32(0.70710678)))

# ---- planted inputs of the soft frame decoder: shared by the host emulation's tests and the GPU tests -----------------------------------
# the coded kinds of tests/chain_host.py's table by name: (tpsap, blk_num, burst type, pieces (offset, length)), type-2 bits, block type
_CODED = [b for b in ch.BLOCKS if b.kind != ch.KIND_BBK]
KINDS = {b.name: (b.tpsap, b.blk, b.train, b.pieces) for b in _CODED}
TYPE2_BITS = {b.name: b.type2 for b in _CODED}
REF_TPSAP = {b.name: b.tpsap for b in _CODED}


def soft_rows_for(lref, kind, rng):
    """int8 rows [n][type345] and their scrambling codes: clean codewords of the reference's encoder at several amplitudes, noisy
    ones, uniform random values, the overflow bound's rows (all +Q, all -Q, alternating) and rows of ties (all zero, sparse)."""
    tpsap = REF_TPSAP[kind]
    n345, n2, n1, a, _ = lref.BLK_PARAM[tpsap]
    rows, codes = [], []
    for i in range(12):
        code = int(rng.integers(0, 1 << 32))
        t5 = lref.lmac_encode(tpsap, rng.integers(0, 2, n1).astype(np.uint8), code)
        clean = (1 - 2 * t5.astype(np.int32))
        amp = (Q, 16, 1, 5)[i % 4]
        rows.append(clean * amp), codes.append(code)
        for sigma in (6.0, 12.0, 20.0):
            rows.append(np.clip(np.rint(clean * 16 + rng.normal(0, sigma, n345)), -Q, Q)), codes.append(code)
    for i in range(24):
        rows.append(rng.integers(-Q, Q + 1, n345)), codes.append(int(rng.integers(0, 1 << 32)))
    alt = np.where(np.arange(n345) % 2 == 0, Q, -Q)
    for r in (np.full(n345, Q), np.full(n345, -Q), alt, -alt, np.zeros(n345)):
        for code in (0, 3, 0xffffffff, int(rng.integers(0, 1 << 32))):
            rows.append(r), codes.append(code)
    for i in range(8):                                     # mostly ties
        r = np.zeros(n345)
        r[rng.integers(0, n345, 6)] = rng.integers(-Q, Q + 1, 6)
        rows.append(r), codes.append(int(rng.integers(0, 1 << 32)))
    return np.array(rows, np.int8), np.array(codes, np.uint32)


class DefinitionEncoder:
    """soft_rows_for's `lref` where the reference is not built: its block parameters, and tests/list_definition.py's transmitter (which
    tests/test_lmac_soft_gpu.py holds against the reference's lmac_encode where that is at hand)."""
    BLK_PARAM = {b.tpsap: (b.type5, b.type2, b.type1, list_definition.BLK[b.tpsap][3], 1) for b in _CODED}         # [3]: the interleaver's a

    @staticmethod
    def lmac_encode(tpsap, type1, code):
        return list_definition.encode(tpsap, type1, code)


def lay_rings(kind, rows, ring=1024, bitnum=None):
    """Every row laid into a ring of its own at the kind's burst positions behind bit number bitnum[j] (None: spread so that rows wrap
    their ring at every offset), the rest of the ring filled with junk -> (rings int8 [n][ring], bit numbers uint32 [n])."""
    tpsap, blk, train, pieces = KINDS[kind]
    n = len(rows)
    bn = (np.arange(n, dtype=np.uint64) * 37 + 0xfffffe00).astype(np.uint32) if bitnum is None else np.ascontiguousarray(bitnum, np.uint32)
    rings = np.random.default_rng(5).integers(-31, 32, (n, ring)).astype(np.int8)
    at = 0
    for off, ln in pieces:
        idx = (bn[:, None].astype(np.int64) + off + np.arange(ln)[None, :]) % ring
        np.put_along_axis(rings, idx, rows[:, at:at + ln], axis=1)
        at += ln
    assert at == rows.shape[1]
    return rings, bn


def quantise_np(sym, prev=FRESH_PREV):
    """The quantiser restated in numpy binary32: sym complex64 [n] -> int8 [2n] (bit 2k: d.re + d.im, bit 2k+1: d.re - d.im of
    d = s[k] conj(s[k-1]); q = clamp(rint(G v), -Q, Q), NaN -> 0)."""
    z = np.ascontiguousarray(sym, np.complex64)
    if z.size == 0:
        return np.zeros(0, np.int8)
    s = z.view(np.float32).reshape(-1, 2)
    p = np.concatenate([np.array([[prev.real, prev.imag]], np.float32), s[:-1]])
    with np.errstate(all="ignore"):
        re = s[:, 0] * p[:, 0] + s[:, 1] * p[:, 1]
        im = s[:, 1] * p[:, 0] - s[:, 0] * p[:, 1]
        v = np.stack([re + im, re - im], axis=1).reshape(-1).astype(np.float32)
        x = np.clip(G * v, np.float32(-Q), np.float32(Q))
        q = np.where(np.isnan(x), np.float32(0), np.rint(x))
    return q.astype(np.int8)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def scramb_seq(ref, code, n):
    seq = np.zeros(n, np.uint8)
    ref.lmac_lib().tetra_scramb_bits(int(code) & 0xffffffff, _p(seq), n)
    return seq


def ref_soft_decode(ref, blk_type, soft5, code):
    """One coded block through the reference chain from soft type-5 values int8 [type345] -> (type-2 bits, crc_ok)."""
    L = ref.lmac_lib()
    L.conv_cch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    n345, n2, n1, a, have_crc = ref.BLK_PARAM[blk_type]
    assert a and have_crc
    t4 = np.zeros(512, np.int8)
    v = np.asarray(soft5, np.int8)[:n345]
    t4[:n345] = np.where(scramb_seq(ref, ref.SCRAMB_INIT if blk_type == ref.TPSAP_T_SB1 else code, n345) != 0, -v, v)
    t3 = np.zeros(512, np.int8)
    L.block_deinterleave(n345, a, _p(t4), _p(t3))
    mother = np.zeros(512 * 4, np.int8)                  # punctured positions: 0
    L.tetra_rcpc_depunct(ref.RCPC_PUNCT_2_3, _p(t3), n345, _p(mother))
    t2 = np.zeros(512, np.uint8)
    L.conv_cch_decode(_p(mother), _p(t2), n2)
    return t2[:n2].copy(), int(L.crc16_ccitt_bits(_p(t2), n1 + 16) == ref.TETRA_CRC_OK)


def channel_rows(ref, oracle, bits, soft, channel, use_soft, sync=None):
    """One channel's whole stream -> {kind: [(channel, bitnum, crc_ok, time on entry, time, type-1 bytes)]} in frame order.  bits: the
    oracle demodulator's bits; soft: the quantiser's value per bit (same numbering).  Frames: the synchroniser (sync(); default the
    burst-synchroniser oracle) a bit per call; tests/chain_host.walk under the reference's clock (tetra_tdma_time_add_tn) and scrambling
    codes (tetra_scramb_get_init).  Every block of a frame carries the time on entry and the time after the SB1."""
    frames, types, bitnums = (sync or oracle.BurstSyncOracle)().feed(bits, chunk=1)

    def decode(f, kind, code):
        b = ch.BLOCK[(int(types[f]), kind)]
        if kind == ch.KIND_BBK or not use_soft:
            return ref.lmac_decode(b.tpsap, ch.cut(frames[f], 0, b.pieces), code)
        return ref_soft_decode(ref, b.tpsap, ch.cut(soft, int(bitnums[f]), b.pieces), code)

    rows = {k: [] for k in range(6)}
    steps = ch.walk(types, ch.ref_clock(ref), lambda f: decode(f, ch.KIND_SB1, 0), ref.scramb_get_init)
    for f, (code, t_rx, t_af, sb1) in enumerate(steps):
        for kind in ch.BURST_KINDS.get(int(types[f]), ()):
            t2, ok = sb1 if kind == ch.KIND_SB1 else decode(f, kind, code)
            rows[kind].append((channel, int(bitnums[f]), int(ok), t_rx, t_af, t2[:ch.TYPE1_BITS[kind]].tobytes()))
    return rows


def oracle_streams(oracle, iq):
    """iq complex64 [C][N] -> per channel the oracle demodulator's bits, and the quantiser's value per bit of its symbols"""
    bits, nb, sym, _ = oracle.process_batch(iq, want_sym=True)
    return [bits[c][:nb[c]] for c in range(len(iq))], [quantise_np(sym[c][:nb[c] // 2]) for c in range(len(iq))]


def stream_rows(ref, oracle, iq, use_soft, sync=None):
    """iq complex64 [C][N] -> rows of every kind as tests/chain_gpu.py's collect gives them (all channels, channel-major), from the oracle
    demodulator's bits and symbols."""
    out = {k: [] for k in range(6)}
    for c, (bits, soft) in enumerate(zip(*oracle_streams(oracle, iq))):
        rows = channel_rows(ref, oracle, bits, soft, c, use_soft, sync)
        for k in out:
            out[k] += rows[k]
    return out
