"""The receive chain's traffic routing (include/ext/tetra_traffic.h) restated on the host, for tests/test_rx_traffic.py (CPU) and
tests/test_rx_traffic_gpu.py: the rule in Python, and the TCH rows a stream must give -- tests/chain_host.py's walk of a channel's
frames under the reference's own decoder, clock and scrambling codes, the AACH under the handle's rule (tests/options_pipeline.py), and
tests/tch_definition.py's / tests/tch_soft_definition.py's chains of the reference's functions on the routed frames.  Nothing of the
product's code runs here.

The rule.  The reference's lower MAC treats the SCH/F block of a burst as traffic when cur_burst.is_traffic is set
(lower_mac/tetra_lower_mac.c:287); the upper MAC sets it from the burst's own ACCESS-ASSIGN: macpdu_decode_access_assign with f18 = 0
(tetra_mac_pdu.c:257-297: hdr = bits 0..1, field1 = bits 2..7; hdr 0 makes field1 an access field, hdr 1..3 the downlink usage marker)
and then is_traffic = dl_usage if dl_usage > 3 else 0 (tetra_upper_mac.c:499-504).  Which timeslot carries which TCH kind is the host's
table; frame 18 is the control frame and never traffic."""
import numpy as np

from tests import chain_host as ch
from tests import options_pipeline as OP
from tests import soft_pipeline as SP
from tests import tch_definition as td
from tests import tch_soft_definition as tsd

TCH_KINDS = (td.TCH_7_2, td.TCH_4_8, td.TCH_2_4)
SOFT, BITERR, AACH_RM3014, AACH_SOFT = OP.SOFT, OP.BITERR, OP.AACH_RM3014, OP.AACH_SOFT
SCHF_PIECES = ch.BLOCK[(ch.TRAIN_NORM_1, ch.KIND_SCH_F)].pieces


def slot_valid(kind, usage):
    return (kind == 0 or kind in TCH_KINDS) and (usage == 0 or 4 <= usage <= 63)


def access_assign(bits):
    """macpdu_decode_access_assign(f18 = 0) as far as the rule needs it: -> the downlink usage marker, or 0 where the PDU carries none"""
    hdr = int(bits[0]) << 1 | int(bits[1])
    field1 = int("".join(str(int(b) & 1) for b in bits[2:8]), 2)
    return field1 if hdr != 0 else 0


def route(frame_type, code, time, slots4, bbk_ok, bbk_bits):
    """Rules (a)..(e) for one frame slot -> the TCH kind its row has, or 0.  slots4: [(kind, usage)] of timeslots 1..4."""
    if int(frame_type) != ch.TRAIN_NORM_1:                  # (a)
        return 0
    if int(code) == 0:                                      # (b)
        return 0
    tn, fn = int(time) & 0xff, (int(time) >> 8) & 0xff
    if not 1 <= tn <= 4 or fn == 18:                        # (c)
        return 0
    kind, usage = slots4[tn - 1]
    if kind not in TCH_KINDS:                               # (d)
        return 0
    if usage != 0:                                          # (e)
        if int(bbk_ok) != 1:
            return 0
        dl_usage = access_assign(bbk_bits)
        is_traffic = dl_usage if dl_usage > 3 else 0        # tetra_upper_mac.c:499-504
        if is_traffic != usage:
            return 0
    return kind


def route_many(frame_type, code, time, slots, bbk_ok, bbk_bits):
    """route() over arrays: slots uint8 [n][4][>= 2] (kind, usage), bbk_bits uint8 [n][>= 8] -> int32 [n]"""
    ft, code, time, ok = (np.asarray(a).astype(np.int64) for a in (frame_type, code, time, bbk_ok))
    slots, bits = np.asarray(slots).astype(np.int64), np.asarray(bbk_bits).astype(np.int64) & 1
    tn, fn = time & 0xff, (time >> 8) & 0xff
    good = (ft == ch.TRAIN_NORM_1) & (code != 0) & (tn >= 1) & (tn <= 4) & (fn != 18)
    at = np.clip(tn - 1, 0, 3)
    rows = np.arange(len(ft))
    kind, usage = slots[rows, at, 0], slots[rows, at, 1]
    good &= (kind >= 8) & (kind <= 10)
    hdr = bits[:, 0] << 1 | bits[:, 1]
    field1 = (bits[:, 2:8] << np.arange(5, -1, -1)[None, :]).sum(axis=1)
    dl_usage = np.where(hdr != 0, field1, 0)
    is_traffic = np.where(dl_usage > 3, dl_usage, 0)
    good &= (usage == 0) | ((ok == 1) & (is_traffic == usage))
    return np.where(good, kind, 0).astype(np.int32)


def clamp(routed, max_rows):
    """-> (routed, kept, dropped)"""
    kept = min(routed, max_rows)
    return routed, kept, routed - kept


def channel_walk(ref, oracle, bits, soft, use_soft):
    """A channel's frames and tests/chain_host.walk over them with the reference's decoder (on the quantiser's values under SOFT), clock
    and scrambling codes -> the walk as tests/list_pipeline.channel_walk gives it."""
    frames, types, bitnums = oracle.BurstSyncOracle().feed(bits, chunk=1)
    b = ch.BLOCK[(ch.TRAIN_SYNC, ch.KIND_SB1)]

    def sb1(f):
        if use_soft:
            return SP.ref_soft_decode(ref, b.tpsap, ch.cut(soft, int(bitnums[f]), b.pieces), 0)
        return ref.lmac_decode(b.tpsap, ch.cut(frames[f], 0, b.pieces), 0)
    steps = list(ch.walk(types, ch.ref_clock(ref), sb1, ref.scramb_get_init))
    codes, t_rx, t_af = (np.array([s[i] for s in steps], dt) for i, dt in enumerate((np.uint32, np.int64, np.int64)))
    return dict(frames=frames, types=types, bitnums=bitnums, codes=codes, t_rx=t_rx, t_af=t_af, sb1=[s[3] for s in steps])


def channel_rows(ref, oracle, bits, soft, channel, slots4, flags=0, walk=None):
    """One channel's whole stream -> {TCH kind: [(channel, bitnum, 1, time on entry, time, type-2 bytes, count word or None)]} in frame
    order.  flags: the handle's create flags, of which SOFT (SB1 and the coded TCH kinds from the quantiser's values), BITERR (the
    count words) and AACH_RM3014 / AACH_SOFT (the row and verdict rule (e) reads) matter."""
    L = ref.lmac_lib()
    use_soft = bool(flags & SOFT)
    walk = walk or channel_walk(ref, oracle, bits, soft, use_soft)
    rule = "ml" if flags & AACH_SOFT else "rm" if flags & AACH_RM3014 else "pass"
    bbk = OP.aach_rows(walk, soft, channel, rule)
    rows = {k: [] for k in TCH_KINDS}
    for f in range(len(walk["types"])):
        ft, bn, code = int(walk["types"][f]), int(walk["bitnums"][f]), int(walk["codes"][f])
        if ft not in ch.BURST_KINDS:
            continue
        ok, _, _, aach = bbk[(ch.KIND_BBK, channel, bn)][:4]
        kind = route(ft, code, walk["t_af"][f], slots4, ok, np.frombuffer(aach, np.uint8))
        if not kind:
            continue
        if use_soft and kind in td.CODED:
            rx = ch.cut(soft, bn, SCHF_PIECES)
            t2 = tsd.decode(L, kind, rx, code)
            word = tsd.biterr_word(L, kind, rx, code, t2) if flags & BITERR else None
        else:
            rx = ch.cut(walk["frames"][f], 0, SCHF_PIECES)
            t2 = td.decode(L, kind, rx, code)
            word = td.biterr_word(L, kind, rx, code, t2) if flags & BITERR and kind in td.CODED else None
        rows[kind].append((channel, bn, 1, int(walk["t_rx"][f]), int(walk["t_af"][f]), t2.tobytes(), word))
    return rows


def stream_rows(ref, oracle, iq, table, flags=0, streams=None):
    """iq complex64 [C][N], table [per channel [(kind, usage)] x 4] -> {TCH kind: rows of all channels, channel-major}"""
    bits, soft = streams or SP.oracle_streams(oracle, iq)
    out = {k: [] for k in TCH_KINDS}
    for c in range(len(iq)):
        rows = channel_rows(ref, oracle, bits[c], soft[c], c, table[c], flags)
        for k in out:
            out[k] += rows[k]
    return out


def table_of(n_channels, entries):
    """{(channel, tn): (kind, usage)} -> [per channel [(kind, usage)] x 4]"""
    t = [[(0, 0)] * 4 for _ in range(n_channels)]
    for (c, tn), v in entries.items():
        t[c][tn - 1] = tuple(v)
    return t


def table_arg(table):
    """-> per channel {tn: (kind, usage)}, as RxChain.set_traffic takes it"""
    return [{tn + 1: v for tn, v in enumerate(slots) if v != (0, 0)} for slots in table]


# ---- the stream of the GPU tests: 4 channels x 40 slots from slot 60 on, so that frames 16, 17, 18, 1 .. 7 occur ------------------------
CHANNELS, SLOTS, SLOT0, SAMPLES, SEED = 4, 40, 60, 20400, 7410
# the mixed table: all three kinds, off slots (and a channel's off timeslot whose transmitter sends SCH/F), gated and ungated entries
MIXED = [[(0, 0), (8, 0), (0, 0), (9, 9)], [(0, 0), (10, 33), (0, 0), (0, 0)], [(0, 0), (9, 0), (0, 0), (10, 0)], [(0, 0), (0, 0), (0, 0), (8, 63)]]


def assert_payloads(rows, tx):
    """every row's type-1 bits are the payload that was sent, as that kind, in the slot its TDMA time names"""
    sent = [sent_by_time(t) for t in tx]
    for k, v in rows.items():
        for r in v:
            kind, pay = sent[r[0]].get(r[4], (None, None))
            assert kind == k and np.frombuffer(r[5], np.uint8)[:len(pay)].tobytes() == pay.tobytes(), (k, r[0], r[1], hex(r[4]))


def codewords():
    from tests import aach_soft_definition as A
    return A.codewords()


def downlink(synth, sent_table, aach=None, esn0_db=None, n_channels=CHANNELS, seed=SEED):
    """Coded downlinks, a different cell per channel, whose traffic timeslots are what sent_table says (table_of's form; what the
    transmitter does, which a test may make differ from the receiver's table) -> (cells, tx (synth.gen_downlink's), iq complex64 [C][N])."""
    cells = [(100 + 7 * c, 1000 + 13 * c, (5 + 3 * c) % 64) for c in range(n_channels)]
    level = {} if esn0_db is None else dict(esn0_db=esn0_db)
    tx = [synth.gen_downlink(SLOTS, seed + c, cell=cells[c], slot0=SLOT0, aach=None if aach is None else aach[c],
                             traffic={tn + 1: v for tn, v in enumerate(sent_table[c]) if v[0]}, aach_codewords=codewords()) for c in range(n_channels)]
    iq = np.stack([synth.gen_channel(SAMPLES, seed + 100 + c, bits=tx[c][0], **level)[0] for c in range(n_channels)])
    return cells, tx, iq


def sent_by_time(tx_c):
    """{packed TDMA time: (kind, type-1 bits)} of one channel's transmitted TCH blocks"""
    out = {}
    for slot, kind, pay in tx_c[1].get("tch", []):
        s = slot + SLOT0
        out[(s % 4 + 1) | ((s // 4) % 18 + 1) << 8 | ((s // 72) % 60 + 1) << 16] = (kind, pay)
    return out
