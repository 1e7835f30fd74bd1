"""What the receive chain with TETRA_RX_FLAG_LIST has to give for a channel's demodulated bits, without any of the product's decoder:
frames from the burst-synchroniser oracle, every coded block decoded and rescued by the numpy definition (tests/list_definition.py),
SB1 first and feeding the SYNC tracker's walk -- tp_sap_udata_ind's SB1 case (a good CRC, rescued ones included, sets the scrambling
code and the clock; the clock steps one timeslot per frame) -- and the other kinds under the code in force.
T = 0 is the chain without the flag."""
import numpy as np

from tests import list_definition as D
from tests import soft_pipeline as sp

CODED_KINDS = (sp.KIND_SB1, sp.KIND_SB2, sp.KIND_NDB1, sp.KIND_NDB2, sp.KIND_SCH_F)
TYPE1 = {sp.KIND_SB1: 60, sp.KIND_SB2: 124, sp.KIND_NDB1: 124, sp.KIND_NDB2: 124, sp.KIND_SCH_F: 268}


def _val(bits, a, n):
    return int("".join(str(int(x)) for x in bits[a:a + n]), 2)


def add_tn(t):
    """One timeslot on [tn, fn, mn], in place: the host build of the tracker's clock (tests/emul/lmac_emul_bind.tdma_advance), which
    tests/test_lmac.py pins to the reference's tetra_tdma_time_add_tn over the whole state space."""
    from tests.emul import lmac_emul_bind
    p = int(lmac_emul_bind.tdma_advance(np.array([t], np.uint32), 1)[0][0])
    t[0], t[1], t[2] = p & 0xff, (p >> 8) & 0xff, p >> 16


def scramb_code(colour, mcc, mnc):
    return ((((colour & 0x3f) | ((mnc & 0x3fff) << 6) | ((mcc & 0x3ff) << 20)) << 2) | 3) & 0xffffffff


def _decode(tpsap, rows, codes, T, soft):
    """rows [n][type345] (bits, or soft values) -> (type-2 bits, crc_ok, rank) by the definition; T = 0: the ML path alone"""
    if len(rows) == 0:
        return np.zeros((0, D.BLK[tpsap][1]), np.uint8), np.zeros(0, np.int32), np.zeros(0, np.int32)
    v3 = D.soft_values(tpsap, rows, codes) if soft else D.hard_values(tpsap, rows, codes)
    d = D.list_decode(tpsap, v3, T, D.START_SOFT if soft else D.START_HARD)
    return d["out"], d["ok"], d["rank"]


def channel_rows(oracle, bits, channel, T, soft=None):
    """-> {(kind, channel, bitnum): (crc_ok, time on entry, time, type-1 bytes, rank, (errors, compared) of tetra_biterr.h on the row's
    final bits)} for the coded kinds of one channel's stream.
    soft: the quantiser's value per bit (same numbering) for the soft route, else None."""
    frames, types, bitnums = oracle.BurstSyncOracle().feed(bits, chunk=1)
    nfr = len(frames)

    def cut(kind, which):
        rows = []
        for f in which:
            _, pieces = sp.PIECES[(int(types[f]), kind)]
            src, at = (frames[f], 0) if soft is None else (soft, int(bitnums[f]))
            rows.append(np.concatenate([src[at + o:at + o + n] for o, n in pieces]))
        return np.array(rows)

    sync = [f for f in range(nfr) if int(types[f]) == sp.TRAIN_SYNC]
    sb1, sb1_ok, sb1_rank = _decode(0, cut(sp.KIND_SB1, sync), np.zeros(len(sync), np.uint32), T, soft is not None)
    at_sync = {f: j for j, f in enumerate(sync)}
    code, phy = 0, [0, 0, 0]
    codes, t_rx, t_af = np.zeros(nfr, np.uint32), np.zeros(nfr, np.int64), np.zeros(nfr, np.int64)
    pack = lambda t: t[0] | (t[1] << 8) | (t[2] << 16)
    for f in range(nfr):
        add_tn(phy)
        t_rx[f] = t_af[f] = pack(phy)
        j = at_sync.get(f)
        if j is not None and sb1_ok[j]:
            b = sb1[j]
            code = scramb_code(_val(b, 4, 6), _val(b, 31, 10), _val(b, 41, 14))
            phy = [_val(b, 10, 2) + 1, _val(b, 12, 5), _val(b, 17, 6)]
            t_af[f] = pack(phy)
        codes[f] = code
    out = {}
    for kind in CODED_KINDS:
        which = [f for f in range(nfr) if kind in sp.BURST_KINDS.get(int(types[f]), ())]
        if kind == sp.KIND_SB1:
            tpsap, rx, t2, ok, rank = 0, cut(kind, which), sb1, sb1_ok, sb1_rank
        else:
            tpsap = sp.PIECES[(int(types[which[0]]), kind)][0] if which else 0
            rx = cut(kind, which)
            t2, ok, rank = _decode(tpsap, rx, codes[which], T, soft is not None)
        for j, f in enumerate(which):
            count = D.count_errors(tpsap, rx[j], int(codes[f]), t2[j], soft is not None)
            out[(kind, channel, int(bitnums[f]))] = (int(ok[j]), int(t_rx[f]), int(t_af[f]), t2[j][:TYPE1[kind]].tobytes(), int(rank[j]), count)
    return out


def rescued_sb1_matters(with_list, without):
    """a block of another kind that lies behind a rescued SB1 and has another verdict, other bits or another time than without the rescue"""
    rescued = [(c, bn) for (k, c, bn), v in with_list.items() if k == sp.KIND_SB1 and v[4] > 0]
    for (k, c, bn), v in with_list.items():
        if k != sp.KIND_SB1 and v[:4] != without[(k, c, bn)][:4] and any(rc == c and rbn <= bn for rc, rbn in rescued):
            return True
    return False
