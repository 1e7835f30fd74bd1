"""The receive chain's soft-decision option (TETRA_RX_FLAG_SOFT) restated on the host from the reference's own programs, for
tests/test_rx_soft.py: oracle symbols -> quantiser (numpy float32) -> the reference's soft decoder, and oracle bits -> the reference's
hard decoder, under the reference's clock and scrambling codes.  Nothing of the product's code runs here.

    soft decode of a block:  sign-descramble (tetra_scramb_bits on zeros gives the sequence) -> block_deinterleave -> tetra_rcpc_depunct
                             onto zeros -> conv_cch_decode (viterbi_cch.c -> osmo_conv.c) -> crc16_ccitt_bits
    hard decode:             ref_binding.lmac_decode (tp_sap_udata_ind's order of the same primitives)
"""
import ctypes as C

import numpy as np

Q, G = 31, np.float32(16.0)                     # csrc/soft_core.hpp
FRESH_PREV = np.complex64(complex(np.float32(0.70710678), np.float32(0.70710678)))
TRAIN_NORM_1, TRAIN_NORM_2, TRAIN_SYNC = 0, 1, 3
# chain kind (TETRA_RX_KIND_*) -> (tpsap, pieces of the burst); per burst type the kinds in tetra_burst_rx_cb's order
KIND_SB1, KIND_BBK, KIND_SB2, KIND_NDB1, KIND_NDB2, KIND_SCH_F = range(6)
PIECES = {
    (TRAIN_SYNC, KIND_SB1): (0, ((94, 120),)), (TRAIN_SYNC, KIND_BBK): (3, ((252, 30),)), (TRAIN_SYNC, KIND_SB2): (1, ((282, 216),)),
    (TRAIN_NORM_2, KIND_BBK): (3, ((230, 14), (266, 16))), (TRAIN_NORM_2, KIND_NDB1): (2, ((14, 216),)), (TRAIN_NORM_2, KIND_NDB2): (2, ((282, 216),)),
    (TRAIN_NORM_1, KIND_BBK): (3, ((230, 14), (266, 16))), (TRAIN_NORM_1, KIND_SCH_F): (5, ((14, 216), (282, 216))),
}
BURST_KINDS = {TRAIN_SYNC: (KIND_SB1, KIND_BBK, KIND_SB2), TRAIN_NORM_2: (KIND_BBK, KIND_NDB1, KIND_NDB2), TRAIN_NORM_1: (KIND_BBK, KIND_SCH_F)}
TYPE1_BITS = (60, 30, 124, 124, 124, 268)

# ---- planted inputs of the soft frame decoder: shared by the host emulation's tests and the GPU tests -----------------------------------
# where a kind's type-5 bits sit in its 510-bit burst (tetra_burst.c:343-393): (tpsap, blk_num, burst type, pieces (offset, length))
KINDS = {
    "sb1": (0, 1, 3, ((94, 120),)),
    "sb2": (1, 2, 3, ((282, 216),)),
    "ndb1": (2, 1, 1, ((14, 216),)),
    "ndb2": (2, 2, 1, ((282, 216),)),
    "schf": (5, 0, 0, ((14, 216), (282, 216))),
}
TYPE2_BITS = {"sb1": 80, "sb2": 144, "ndb1": 144, "ndb2": 144, "schf": 288}
REF_TPSAP = {"sb1": 0, "sb2": 1, "ndb1": 2, "ndb2": 2, "schf": 5}


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
    BLK_PARAM = {0: (120, 80, 60, 11, 1), 1: (216, 144, 124, 101, 1), 2: (216, 144, 124, 101, 1), 5: (432, 288, 268, 103, 1)}

    @staticmethod
    def lmac_encode(tpsap, type1, code):
        from tests import list_definition
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


class _TdmaTime(C.Structure):
    """struct tetra_tdma_time (src/decoder/src/tetra_tdma.h:6-12)"""
    _fields_ = [("hn", C.c_uint16), ("sn", C.c_uint32), ("tn", C.c_uint32), ("fn", C.c_uint32), ("mn", C.c_uint32)]


def _bits_val(t2, a, n):
    return int("".join(str(int(x)) for x in t2[a:a + n]), 2)


def channel_rows(ref, oracle, bits, soft, channel, use_soft):
    """One channel's whole stream -> {kind: [(channel, bitnum, crc_ok, time on entry, time, type-1 bytes)]} in frame order.  bits: the
    oracle demodulator's bits; soft: the quantiser's value per bit (same numbering).  Frames: the burst-synchroniser oracle a bit per
    call; per frame the clock steps (tetra_tdma_time_add_tn, the reference's), SB1 first: a good CRC sets the clock and the
    scrambling code (tetra_scramb_get_init) every other block of the burst and every later one is descrambled with."""
    add_tn = ref.lib().tetra_tdma_time_add_tn
    add_tn.argtypes = [C.POINTER(_TdmaTime), C.c_uint32]
    add_tn.restype = None
    frames, types, bitnums = oracle.BurstSyncOracle().feed(bits, chunk=1)
    rows = {k: [] for k in range(6)}
    code, phy = 0, _TdmaTime()
    pack = lambda t: t.tn | (t.fn << 8) | (t.mn << 16)
    for fr, ft, bn in zip(frames, types, bitnums):
        add_tn(C.byref(phy), 1)
        t_rx = t_af = pack(phy)
        pending = []
        for kind in BURST_KINDS.get(int(ft), ()):
            tpsap, pieces = PIECES[(int(ft), kind)]
            hard5 = np.concatenate([fr[o:o + n] for o, n in pieces])
            if kind == KIND_BBK or not use_soft:
                t2, ok = ref.lmac_decode(tpsap, hard5, code)
            else:
                soft5 = np.concatenate([soft[int(bn) + o:int(bn) + o + n] for o, n in pieces])
                t2, ok = ref_soft_decode(ref, tpsap, soft5, code)
            if kind == KIND_SB1 and ok:                  # tetra_lower_mac.c:246-275
                code = ref.scramb_get_init(_bits_val(t2, 31, 10), _bits_val(t2, 41, 14), _bits_val(t2, 4, 6))
                phy.tn, phy.fn, phy.mn = _bits_val(t2, 10, 2) + 1, _bits_val(t2, 12, 5), _bits_val(t2, 17, 6)
                t_af = pack(phy)
            pending.append((kind, ok, t2[:TYPE1_BITS[kind]].tobytes()))
        # (a SYNC burst's SB1 comes first: its AACH and SB2 are handled under ITS code.)  Every block of the frame carries the time on
        # entry and the time after the SB1
        for kind, ok, t1 in pending:
            rows[kind].append((channel, int(bn), int(ok), t_rx, t_af, t1))
    return rows


def stream_rows(ref, oracle, iq, use_soft):
    """iq complex64 [C][N] -> rows of every kind as tests/test_rx.py's _collect gives them (all channels, channel-major), from the oracle
    demodulator's bits and symbols."""
    bits, nb, sym, _ = oracle.process_batch(iq, want_sym=True)
    out = {k: [] for k in range(6)}
    for c in range(len(iq)):
        soft = quantise_np(sym[c][:nb[c] // 2])
        rows = channel_rows(ref, oracle, bits[c][:nb[c]], soft, c, use_soft)
        for k in out:
            out[k] += rows[k]
    return out
