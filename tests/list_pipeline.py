"""What the receive chain with TETRA_RX_FLAG_LIST has to give for a channel's demodulated bits, without any of the product's decoder:
frames from the burst-synchroniser oracle, every coded block decoded and rescued by the numpy definition (tests/list_definition.py),
SB1 first and feeding the SYNC tracker's walk -- tp_sap_udata_ind's SB1 case (a good CRC, rescued ones included, sets the scrambling
code and the clock; the clock steps one timeslot per frame) -- and the other kinds under the code in force.
T = 0 is the chain without the flag."""
import numpy as np

from tests import chain_host as ch
from tests import list_definition as D

CODED_KINDS = ch.CODED_KINDS


def scramb_code(colour, mcc, mnc):
    return ((((colour & 0x3f) | ((mnc & 0x3fff) << 6) | ((mcc & 0x3ff) << 20)) << 2) | 3) & 0xffffffff


def _decode(tpsap, rows, codes, T, soft):
    """rows [n][type345] (bits, or soft values) -> (type-2 bits, crc_ok, rank) by the definition; T = 0: the ML path alone"""
    if len(rows) == 0:
        return np.zeros((0, D.BLK[tpsap][1]), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32)
    v3 = D.soft_values(tpsap, rows, codes) if soft else D.hard_values(tpsap, rows, codes)
    d = D.list_decode(tpsap, v3, T, D.START_SOFT if soft else D.START_HARD)
    return d["out"], d["ok"], d["rank"]


def channel_rows(oracle, bits, channel, T, soft=None, sync=None):
    """-> {(kind, channel, bitnum): (crc_ok, time on entry, time, type-1 bytes, rank, (errors, compared) of tetra_biterr.h on the row's
    final bits)} for the coded kinds of one channel's stream.
    soft: the quantiser's value per bit (same numbering) for the soft route, else None.  sync: the synchroniser (sync(); default the
    burst-synchroniser oracle), as tests/soft_pipeline.channel_rows takes it.  The SB1s are decoded as one batch ahead of
    tests/chain_host.walk (they need no code), which runs under the host build of the tracker's clock and the numpy scramb_code."""
    return channel_walk(oracle, bits, channel, T, soft, sync)[0]


def channel_walk(oracle, bits, channel, T, soft=None, sync=None):
    """channel_rows, and the walk behind it -> (the rows, dict: frames uint8 [n][510], types, bitnums, and per frame the scrambling code in
    force behind its SB1, the packed time on entry and after the SB1, and the SB1's answer (type-2 bits, crc_ok) or None)."""
    frames, types, bitnums = (sync or oracle.BurstSyncOracle)().feed(bits, chunk=1)
    nfr = len(frames)

    def cut(kind, which):
        if soft is None:
            return np.array([ch.cut(frames[f], 0, ch.BLOCK[(int(types[f]), kind)].pieces) for f in which])
        return np.array([ch.cut(soft, int(bitnums[f]), ch.BLOCK[(int(types[f]), kind)].pieces) for f in which])

    sync = [f for f in range(nfr) if int(types[f]) == ch.TRAIN_SYNC]
    sb1, sb1_ok, sb1_rank = _decode(0, cut(ch.KIND_SB1, sync), np.zeros(len(sync), np.uint32), T, soft is not None)
    at_sync = {f: j for j, f in enumerate(sync)}
    steps = list(ch.walk(types, ch.host_clock, lambda f: (sb1[at_sync[f]], sb1_ok[at_sync[f]]), lambda mcc, mnc, colour: scramb_code(colour, mcc, mnc)))
    codes, t_rx, t_af = (np.array([s[i] for s in steps], dt) for i, dt in enumerate((np.uint32, np.int64, np.int64)))
    out = {}
    for kind in CODED_KINDS:
        which = [f for f in range(nfr) if kind in ch.BURST_KINDS.get(int(types[f]), ())]
        tpsap, rx = ch.BY_KIND[kind].tpsap, cut(kind, which)
        t2, ok, rank = (sb1, sb1_ok, sb1_rank) if kind == ch.KIND_SB1 else _decode(tpsap, rx, codes[which], T, soft is not None)
        for j, f in enumerate(which):
            count = D.count_errors(tpsap, rx[j], int(codes[f]), t2[j], soft is not None)
            out[(kind, channel, int(bitnums[f]))] = (int(ok[j]), int(t_rx[f]), int(t_af[f]), t2[j][:ch.TYPE1_BITS[kind]].tobytes(), int(rank[j]), count)
    return out, dict(frames=frames, types=types, bitnums=bitnums, codes=codes, t_rx=t_rx, t_af=t_af, sb1=[s[3] for s in steps])


def rescued_sb1_matters(with_list, without):
    """a block of another kind that lies behind a rescued SB1 and has another verdict, other bits or another time than without the rescue"""
    rescued = [(c, bn) for (k, c, bn), v in with_list.items() if k == ch.KIND_SB1 and v[4] > 0]
    for (k, c, bn), v in with_list.items():
        if k != ch.KIND_SB1 and v[:4] != without[(k, c, bn)][:4] and any(rc == c and rbn <= bn for rc, rbn in rescued):
            return True
    return False
