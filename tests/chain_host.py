"""What the receive chain must deliver, stated once on the host: the table of the block kinds, the SYNC PDU's fields, the two clocks,
the walk over a channel's frames as tp_sap_udata_ind does it, the downlink streams of the chain tests and the row format of their
fixtures.  The pipelines (tests/soft_pipeline.py, tests/list_pipeline.py, tests/aach_soft_pipeline.py) bring their own decoders and
scrambling-code rules; only the order of events is shared.  Nothing of the product's code runs here except the host build of the
tracker's clock, which host_clock names."""
import collections
import ctypes as C
import os

import numpy as np

TRAIN_NORM_1, TRAIN_NORM_2, TRAIN_SYNC = 0, 1, 3
KIND_SB1, KIND_BBK, KIND_SB2, KIND_NDB1, KIND_NDB2, KIND_SCH_F = range(6)             # TETRA_RX_KIND_*

# ---- the block kinds ---------------------------------------------------------------------------------------------------------------------
# One row per block of a burst, per burst type in tetra_burst_rx_cb's order (tetra_burst.c:343-393): where its type-5 bits lie in the
# 510-bit burst as pieces (offset, length), and its type-2 / type-1 bit counts.  The AACH (BBK) is handed on uncoded: 30 bits throughout.
Block = collections.namedtuple("Block", "name kind tpsap blk train pieces type2 type1")
Block.type5 = property(lambda b: sum(n for _, n in b.pieces))
_AACH_SYNC, _AACH_NORM = ((252, 30),), ((230, 14), (266, 16))
BLOCKS = (
    Block("sb1", KIND_SB1, 0, 1, TRAIN_SYNC, ((94, 120),), 80, 60),
    Block("bbk", KIND_BBK, 3, 0, TRAIN_SYNC, _AACH_SYNC, 30, 30),
    Block("sb2", KIND_SB2, 1, 2, TRAIN_SYNC, ((282, 216),), 144, 124),
    Block("bbk", KIND_BBK, 3, 0, TRAIN_NORM_2, _AACH_NORM, 30, 30),
    Block("ndb1", KIND_NDB1, 2, 1, TRAIN_NORM_2, ((14, 216),), 144, 124),
    Block("ndb2", KIND_NDB2, 2, 2, TRAIN_NORM_2, ((282, 216),), 144, 124),
    Block("bbk", KIND_BBK, 3, 0, TRAIN_NORM_1, _AACH_NORM, 30, 30),
    Block("schf", KIND_SCH_F, 5, 0, TRAIN_NORM_1, ((14, 216), (282, 216)), 288, 268),
)
BLOCK = {(b.train, b.kind): b for b in BLOCKS}                                        # (burst type, kind) -> its row
BURST_KINDS = {t: tuple(b.kind for b in BLOCKS if b.train == t) for t in (TRAIN_SYNC, TRAIN_NORM_2, TRAIN_NORM_1)}
BY_KIND = {b.kind: b for b in BLOCKS}                                                 # kind -> a row (the AACH's: its sizes only)
KIND_NAMES = {b.kind: b.name for b in BLOCKS}
CODED_KINDS = tuple(k for k in range(6) if k != KIND_BBK)
TYPE1_BITS = tuple(BY_KIND[k].type1 for k in range(6))
PACKED_BYTES = tuple((n + 7) // 8 for n in TYPE1_BITS)                                # a type-1 row packed 8 bits a byte


def cut(src, at, pieces):
    """a block's type-5 values out of src (a burst's bits with at = 0, or a stream with at = the burst's bit number)"""
    return np.concatenate([src[at + o:at + o + n] for o, n in pieces])


def sync_pdu_fields(t2):
    """-> (mcc, mnc, colour code, tn, fn, mn) of a SYNC PDU's bits (tetra_lower_mac.c:246-275; the PDU carries tn - 1)"""
    val = lambda a, n: int("".join(str(int(x)) for x in t2[a:a + n]), 2)
    return val(31, 10), val(41, 14), val(4, 6), val(10, 2) + 1, val(12, 5), val(17, 6)


# ---- the clock: (tn, fn, mn) -> (tn, fn, mn) one timeslot later --------------------------------------------------------------------------
class TdmaTime(C.Structure):
    """struct tetra_tdma_time (src/decoder/src/tetra_tdma.h:6-12)"""
    _fields_ = [("hn", C.c_uint16), ("sn", C.c_uint32), ("tn", C.c_uint32), ("fn", C.c_uint32), ("mn", C.c_uint32)]


def ref_add_tn(ref):
    """The reference's own tetra_tdma_time_add_tn (oracle/_ref: src/decoder/src/tetra_tdma.c compiled where it lies)."""
    add_tn = ref.lib().tetra_tdma_time_add_tn
    add_tn.argtypes = [C.POINTER(TdmaTime), C.c_uint32]
    add_tn.restype = None
    return add_tn


def ref_clock(ref):
    add_tn = ref_add_tn(ref)

    def step(t):
        s = TdmaTime(tn=t[0], fn=t[1], mn=t[2])
        add_tn(C.byref(s), 1)
        return s.tn, s.fn, s.mn
    return step


def host_clock(t):
    """The host build of the tracker's clock (tests/emul/lmac_emul_bind.tdma_advance), which tests/test_lmac.py pins to the reference's
    tetra_tdma_time_add_tn over the whole state space."""
    from tests.emul import lmac_emul_bind
    p = int(lmac_emul_bind.tdma_advance(np.array([t], np.uint32), 1)[0][0])
    return p & 0xff, (p >> 8) & 0xff, p >> 16


# ---- the walk -----------------------------------------------------------------------------------------------------------------------------
def walk(types, clock, sb1, code_of):
    """A channel's frames in order (types: the burst type of each, from whatever synchroniser) -> per frame (scrambling code in force,
    packed TDMA time on entry, packed time after the SB1, sb1's answer or None): tp_sap_udata_ind's order of events.  The clock steps
    one timeslot per frame; a SYNC burst's SB1 comes first -- sb1(f) -> (its type-2 bits, crc_ok); SB1 is descrambled with the fixed
    code, so it needs none -- and a good CRC sets the clock and, by code_of(mcc, mnc, colour), the code for the burst's other blocks
    and every later frame."""
    pack = lambda t: t[0] | (t[1] << 8) | (t[2] << 16)
    code, t = 0, (0, 0, 0)
    for f, ft in enumerate(types):
        t = clock(t)
        t_rx = t_af = pack(t)
        got = sb1(f) if int(ft) == TRAIN_SYNC else None
        if got is not None and got[1]:
            mcc, mnc, colour, tn, fn, mn = sync_pdu_fields(got[0])
            code, t = code_of(mcc, mnc, colour), (tn, fn, mn)
            t_af = pack(t)
        yield code, t_rx, t_af, got


# ---- the streams ---------------------------------------------------------------------------------------------------------------------------
def downlink_batch(synth, Cn, nslots, N, seed, esn0_db=None, aach=None):
    """Coded downlinks with every block kind, a different cell per channel -> (cells, tx (synth.gen_downlink's), iq complex64 [Cn][N]).
    esn0_db None: the synth's default level; aach: per channel the AACH bits of every slot (None: the synth's own)."""
    cells = [(100 + 7 * c, 1000 + 13 * c, (5 + 3 * c) % 64) for c in range(Cn)]
    level = {} if esn0_db is None else dict(esn0_db=esn0_db)
    tx = [synth.gen_downlink(nslots, seed + c, cell=cells[c], aach=None if aach is None else aach[c]) for c in range(Cn)]
    iq = np.stack([synth.gen_channel(N, seed + 100 + c, bits=tx[c][0], **level)[0] for c in range(Cn)])
    return cells, tx, iq


def noisy_batch(synth, Cn, nslots, N, seed):
    """The same, with the last two channels at low Es/N0 so that some blocks fail their CRC."""
    cells, tx, iq = downlink_batch(synth, Cn, nslots, N, seed)
    rng = np.random.default_rng(seed)
    for c in (Cn - 2, Cn - 1):
        sigma = np.sqrt(np.mean(np.abs(iq[c]) ** 2) / 10 ** (6.0 / 10) / 2)
        iq[c] = iq[c] + (sigma * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    return cells, tx, iq


# The operating point: one second of five coded downlinks.  At Es/N0 = 11 dB, from the reference-only pipeline on the CPU:
# hard decisions leave 21 of 118 SCH/F blocks CRC-bad, soft decisions 12 -- the rows of tests/golden/rx_soft_golden.npz.
OP_CHANNELS, OP_SLOTS, OP_SAMPLES, OP_SEED = 5, 71, 36000, 9000
OP_SCHF = {"hard": (118, 97), "soft": (118, 106)}            # (rows, CRC-good rows) at 11 dB
RX_SOFT_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rx_soft_golden.npz")


def operating_point(synth, esn0_db):
    return downlink_batch(synth, OP_CHANNELS, OP_SLOTS, OP_SAMPLES, OP_SEED, esn0_db)


# ---- fixture rows: {kind: [(channel, bitnum, crc_ok, time on entry, time, type-1 bytes)]} -------------------------------------------------
def rows_to_arrays(rows, n1):
    return dict(label=np.array([r[:5] for r in rows], np.int64).reshape(-1, 5),
                type1=np.frombuffer(b"".join(r[5] for r in rows), np.uint8).reshape(-1, n1))


def golden_rows(path, name):
    """{kind: rows} of a fixture written with rows_to_arrays, as tests/soft_pipeline.py's stream_rows returns them"""
    g = np.load(path)
    return {k: [tuple(int(x) for x in lab) + (t1.tobytes(),) for lab, t1 in zip(g["%s_%d_label" % (name, k)], g["%s_%d_type1" % (name, k)])]
            for k in range(6)}
