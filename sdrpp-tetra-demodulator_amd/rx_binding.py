"""ctypes binding of the receive chain behind one handle (include/tetra_rx.h)."""
import ctypes as C
import functools

import numpy as np

from . import binding as B
from ._ffi import P, TetraDemodError, call, check, declare, i32, i64, ptr, size_t, stream_ptr, u64, vp
from .binding import load_library
from .bsync_binding import BsyncState, BsyncTolerance, tolerance_arg

KIND_SB1, KIND_BBK, KIND_SB2, KIND_NDB1, KIND_NDB2, KIND_SCH_F = range(6)
N_KINDS = 6
FLAG_ONE_STREAM = 1
FLAG_AACH_RM3014 = 2          # TETRA_RX_FLAG_AACH_RM3014
FLAG_SOFT = 8                 # TETRA_RX_FLAG_SOFT: the coded kinds decoded from soft values (4 is no flag)
FLAG_BITERR = 32              # TETRA_RX_FLAG_BITERR: channel bit-error counts per coded block, link figures per channel (tetra_biterr.h)
FLAG_LIST = 512               # TETRA_RX_FLAG_LIST: CRC-aided list decoding of the CRC-failed coded blocks (ext/tetra_list.h)
FLAG_SYNC_TOLERANT = 128      # TETRA_RX_FLAG_SYNC_TOLERANT: the synchroniser's tolerant lock with {3, 5, 16} (ext/tetra_sync_tol.h)
FLAG_AACH_SOFT = 1024         # TETRA_RX_FLAG_AACH_SOFT: the AACH by maximum likelihood on the soft values (ext/tetra_aach_soft.h); needs FLAG_SOFT
AACH_UNDECODABLE = 0xFF       # TETRA_AACH_UNDECODABLE


class RxConfig(C.Structure):
    _fields_ = [("demod", B.Config), ("kinds", C.c_int32), ("flags", C.c_int32)]


class RxBlock(C.Structure):
    _fields_ = [("channel", C.c_int32), ("frame_slot", C.c_int32), ("bitnum", C.c_uint32), ("tdma_time_rx", C.c_uint32),
                ("tdma_time", C.c_uint32), ("crc_ok", C.c_int32)]


BLOCK_DTYPE = np.dtype([("channel", "<i4"), ("frame_slot", "<i4"), ("bitnum", "<u4"), ("tdma_time_rx", "<u4"), ("tdma_time", "<u4"),
                        ("crc_ok", "<i4")])


class CellState(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("scramb_init", "colour_code", "mcc", "mnc", "tcd_tn", "tcd_fn", "tcd_mn", "phy_tn", "phy_fn",
                                          "phy_mn")]


class Link(C.Structure):
    """tetra_rx_link_t."""
    _fields_ = [("bits", C.c_uint64), ("bit_errors", C.c_uint64), ("blocks", C.c_uint32), ("blocks_crc_bad", C.c_uint32)]


# include/tetra_rx.h
SIGNATURES = {
    "tetra_rx_default_config": (i32, [P(RxConfig)]),
    "tetra_rx_create": (i32, [P(RxConfig), P(vp)]),
    "tetra_rx_destroy": (i32, [vp]),
    "tetra_rx_reset": (i32, [vp]),
    "tetra_rx_process_device": (i32, [vp, vp, i32, vp]),
    "tetra_rx_process": (i32, [vp, vp, i32]),
    "tetra_rx_wait": (i32, [vp]),
    "tetra_rx_max_rows": (i32, [vp]),
    "tetra_rx_type1_bits": (i32, [i32]),
    "tetra_rx_fetch": (i32, [vp, i32, i32, vp, vp, i32, i32, P(i32)]),
    "tetra_rx_rows_device": (i32, [vp, i32, i32, P(vp), P(i32), P(vp), P(vp), vp]),
    "tetra_rx_get_cell": (i32, [vp, i32, i32, P(CellState)]),
    "tetra_rx_get_sync_state": (i32, [vp, i32, i32, P(BsyncState)]),
    "tetra_rx_bits_device": (i32, [vp, i32, P(vp), P(i32), P(vp), vp]),
    "tetra_rx_demod": (vp, [vp]),
    "tetra_rx_stage_ms": (i32, [vp, P(C.c_float * 4)]),
}
# include/tetra_rx_out.h (the one-step hand-off of a call's blocks)
OUT_SIGNATURES = {
    "tetra_rx_out_bound": (i32, [vp, i32, i32, P(u64)]),
    "tetra_rx_out_enqueue": (i32, [vp, i32, i32, i32, vp, u64, P(i64)]),
    "tetra_rx_out_query": (i32, [vp, i64]),
    "tetra_rx_out_wait": (i32, [vp, i64]),
    "tetra_rx_out_host_alloc": (vp, [size_t]),
    "tetra_rx_out_host_free": (None, [vp]),
    "tetra_rx_out_view": (i32, [vp, u64, i32, P(vp), P(vp), P(i32), P(i32)]),
    "tetra_rx_unpack_bits": (i32, [vp, i32, i32, i32, vp, i32]),
}
# include/tetra_retune.h (resets of single channels while the stream runs): the chain's share
RETUNE_SIGNATURES = {"tetra_rx_reset_channels_device": (i32, [vp, vp, i32, vp])}
# include/tetra_aach.h (the AACH decoded with its Reed-Muller code): the chain's share
AACH_SIGNATURES = {"tetra_rx_fetch_aach_dist": (i32, [vp, i32, vp, i32, P(i32)])}
# include/ext/tetra_biterr.h (channel bit-error counts): the chain's share
BITERR_ABI = {
    "tetra_rx_fetch_biterr": (i32, [vp, i32, i32, vp, i32, P(i32)]),
    "tetra_rx_biterr_device": (i32, [vp, i32, i32, P(vp), vp]),
    "tetra_rx_get_link": (i32, [vp, i32, i32, P(Link)]),
}
# include/ext/tetra_sync_tol.h (the synchroniser's tolerant lock): the chain's share
SYNC_TOL_ABI = {
    "tetra_rx_set_sync_tolerance": (i32, [vp, P(BsyncTolerance)]),
    "tetra_rx_get_sync_misses": (i32, [vp, i32, i32, vp]),
}
# include/ext/tetra_list.h (CRC-aided list decoding): the chain's share
LIST_ABI = {
    "tetra_rx_set_list_candidates": (i32, [vp, i32]),
    "tetra_rx_fetch_list_rank": (i32, [vp, i32, i32, vp, i32, P(i32)]),
    "tetra_rx_list_rank_device": (i32, [vp, i32, i32, P(vp), vp]),
}
# include/ext/tetra_aach_soft.h (the AACH by maximum likelihood on the soft values): the chain's share
AACH_SOFT_ABI = {
    "tetra_rx_set_aach_min_margin": (i32, [vp, i32]),
    "tetra_rx_fetch_aach_margin": (i32, [vp, i32, vp, i32, P(i32)]),
}
# include/ext/tetra_handover.h (a restarted channel inherits frame timing, cell and clock from a donor): the chain's share
class HandoverParams(C.Structure):
    _fields_ = [("window", C.c_int32), ("max_slots", C.c_int32)]


class HandoverStatus(C.Structure):
    _fields_ = [("state", C.c_int32), ("slots_waited", C.c_int32), ("offset", C.c_int32)]


HANDOVER_NONE, HANDOVER_PENDING, HANDOVER_LOCKED, HANDOVER_EXPIRED, HANDOVER_REFUSED = range(5)
HANDOVER_DEFAULT_WINDOW, HANDOVER_DEFAULT_MAX_SLOTS = 8, 72
SYNC_STATE_ASSIST = 3         # TETRA_BSYNC_STATE_ASSIST
HANDOVER_ABI = {
    "tetra_rx_handover_channels_device": (i32, [vp, vp, vp, i32, P(HandoverParams), vp]),
    "tetra_rx_get_handover": (i32, [vp, i32, i32, P(HandoverStatus)]),
}


def handover_params_arg(window, max_slots):
    """None, None -> NULL (the header's defaults); else the struct with the default for whichever is None."""
    if window is None and max_slots is None:
        return None
    return C.byref(HandoverParams(HANDOVER_DEFAULT_WINDOW if window is None else int(window),
                                  HANDOVER_DEFAULT_MAX_SLOTS if max_slots is None else int(max_slots)))


# include/ext/tetra_gap.h (channels restarted after missing samples keep frame timing, cell and clock): the chain's share
GAP_DEFAULT_WINDOW, GAP_DEFAULT_MAX_SLOTS, GAP_MAX_ELAPSED_BITS = 8, 72, (1 << 31) - 1
GAP_ABI = {"tetra_rx_resume_channels_device": (i32, [vp, vp, i32, i64, P(HandoverParams), vp])}


def gap_params_arg(window, max_slots):
    """handover_params_arg with the gap header's defaults."""
    if window is None and max_slots is None:
        return None
    return C.byref(HandoverParams(GAP_DEFAULT_WINDOW if window is None else int(window), GAP_DEFAULT_MAX_SLOTS if max_slots is None else int(max_slots)))


# include/ext/tetra_rx_out_ext.h (the opt-in row extras and per-channel state through the one-step hand-off)
OUT_EXT_ABI = {
    "tetra_rx_out_bound_ext": (i32, [vp, i32, i32, i32, P(u64)]),
    "tetra_rx_out_enqueue_ext": (i32, [vp, i32, i32, i32, i32, vp, u64, P(i64)]),
    "tetra_rx_out_set_snapshot": (i32, [vp, i32]),
    "tetra_rx_out_view_ext": (i32, [vp, u64, i32, P(vp), P(vp), P(vp), P(i32)]),
    "tetra_rx_out_view_channels": (i32, [vp, u64, P(vp), P(vp), P(vp), P(vp), P(i32)]),
}
# include/ext/tetra_rx_out_rows.h (the delivery's launches over rows the caller provides)
class OutRows(C.Structure):
    """tetra_rx_out_rows_t."""
    _fields_ = [("kind", C.c_int32), ("type2_stride", C.c_int32), ("d_type2", vp), ("d_crc_ok", vp), ("d_blocks", vp), ("d_n_rows", vp),
                ("d_biterr", vp), ("d_rank", vp)]


OUT_ROWS_ABI = {
    "tetra_rx_out_rows_workspace_bytes": (size_t, [i32]),
    "tetra_rx_out_write_rows_device": (i32, [P(OutRows), i32, i32, i32, i32, i64, vp, u64, vp, size_t, vp]),
}
RX_OUT_ROWS_EXPORTS = list(OUT_ROWS_ABI)
# include/ext/tetra_traffic.h (the traffic slots the host names, decoded as TCH blocks)
TCH_7_2, TCH_4_8, TCH_2_4 = 8, 9, 10          # TETRA_LMAC_T_TCH_*
TRAFFIC_TYPE2_BITS = {TCH_7_2: 432, TCH_4_8: 292, TCH_2_4: 148}
TRAFFIC_TYPE1_BITS = {TCH_7_2: 432, TCH_4_8: 288, TCH_2_4: 144}
TRAFFIC_STRIDE = {TCH_7_2: 432, TCH_4_8: 296, TCH_2_4: 152}
TRAFFIC_SLOT_DTYPE = np.dtype([("kind", "u1"), ("usage", "u1"), ("pad", "u1", (2,))])          # tetra_rx_traffic_slot_t
TRAFFIC_ABI = {
    "tetra_rx_traffic_enable": (i32, [vp, i32]),
    "tetra_rx_set_traffic": (i32, [vp, i32, i32, vp, vp]),
    "tetra_rx_get_traffic": (i32, [vp, i32, i32, vp]),
    "tetra_rx_fetch_traffic": (i32, [vp, i32, i32, vp, vp, i32, i32, vp, P(i32), P(i32)]),
    "tetra_rx_traffic_rows_device": (i32, [vp, i32, i32, P(vp), P(i32), P(vp), P(vp), P(vp), vp]),
}
RX_TRAFFIC_EXPORTS = list(TRAFFIC_ABI)


def traffic_table_arg(table):
    """A traffic table as tetra_rx_set_traffic takes it: a TRAFFIC_SLOT_DTYPE array [n][4] as it is; else per channel {tn: kind} or
    {tn: (kind, usage)} for the timeslots 1..4 that carry traffic (None or {}: none)."""
    if isinstance(table, np.ndarray) and table.dtype == TRAFFIC_SLOT_DTYPE:
        return np.ascontiguousarray(table).reshape(-1, 4)
    t = np.zeros((len(table), 4), TRAFFIC_SLOT_DTYPE)
    for c, slots in enumerate(table):
        for tn, v in (slots or {}).items():
            if not 1 <= int(tn) <= 4:
                raise ValueError("timeslots are 1..4")
            kind, usage = v if isinstance(v, tuple) else (v, 0)
            t[c, int(tn) - 1]["kind"], t[c, int(tn) - 1]["usage"] = int(kind), int(usage)
    return t


RX_EXPORTS, RX_OUT_EXPORTS = list(SIGNATURES), list(OUT_SIGNATURES)
RX_RETUNE_EXPORTS, RX_AACH_EXPORTS, RX_BITERR_EXPORTS = list(RETUNE_SIGNATURES), list(AACH_SIGNATURES), list(BITERR_ABI)
RX_OUT_EXT_EXPORTS = list(OUT_EXT_ABI)
RX_HANDOVER_EXPORTS = list(HANDOVER_ABI)
RX_GAP_EXPORTS = list(GAP_ABI)


@functools.lru_cache(None)
def _lib():
    # (a TETRA_DEMOD_LIB override may be an older build without the hand-off, retune and AACH additions)
    return declare(load_library(), {**SIGNATURES, **OUT_SIGNATURES, **RETUNE_SIGNATURES, **AACH_SIGNATURES, **BITERR_ABI, **SYNC_TOL_ABI, **LIST_ABI,
                                    **OUT_EXT_ABI, **HANDOVER_ABI, **OUT_ROWS_ABI, **AACH_SOFT_ABI, **GAP_ABI, **TRAFFIC_ABI},
                   optional=RX_OUT_EXPORTS + RX_RETUNE_EXPORTS + RX_AACH_EXPORTS + RX_BITERR_EXPORTS + list(SYNC_TOL_ABI) + list(LIST_ABI) +
                   RX_OUT_EXT_EXPORTS + RX_HANDOVER_EXPORTS + RX_OUT_ROWS_EXPORTS + list(AACH_SOFT_ABI) + RX_GAP_EXPORTS + RX_TRAFFIC_EXPORTS)


def type1_bits(kind):
    return int(_lib().tetra_rx_type1_bits(int(kind)))


class RxChain:
    """IQ in, decoded type-1 blocks + CRC + TDMA time + cell state out, for C channels on one GPU: demodulator -> burst
    synchroniser -> demultiplexer -> lower-MAC decoder -> SYNC-PDU tracker, ordered and buffered by the library."""

    def __init__(self, n_channels=1, max_samples=36000, layout=B.LAYOUT_CHANNEL_MAJOR, device=-1, kinds=0, flags=0, demod_flags=0, **params):
        self._lib = _lib()
        cfg = RxConfig()
        call(self._lib.tetra_rx_default_config, C.byref(cfg))
        cfg.demod.n_channels, cfg.demod.max_samples, cfg.demod.layout, cfg.demod.device = n_channels, max_samples, layout, device
        cfg.demod.flags = demod_flags
        for k, v in params.items():
            if k not in B.PARAMS:
                raise TypeError("unknown parameter %r" % k)
            setattr(cfg.demod, k, v)
        cfg.kinds, cfg.flags = kinds, flags
        self.n_channels, self.max_samples = n_channels, max_samples
        h = C.c_void_p()
        call(self._lib.tetra_rx_create, C.byref(cfg), C.byref(h))
        self._h = h
        self.max_rows = int(self._lib.tetra_rx_max_rows(h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tetra_rx_destroy(self._h)          # synchronises the device: no delivery still writes into the pool
            self._h = None
        self._close_pool()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        call(self._lib.tetra_rx_reset, self._h)

    def reset_channels(self, channels, stream=None):
        """tetra_rx_reset_channels_device: the listed channels start afresh from the next process call on, everything else stays;
        enqueued on `stream`, not waited for."""
        ch = np.ascontiguousarray(np.asarray(channels, np.int64).astype(np.int32).reshape(-1))
        call(self._lib.tetra_rx_reset_channels_device, self._h, ptr(ch) if ch.size else None, int(ch.size), stream_ptr(stream))

    def handover_channels(self, channels, donors, window=None, max_slots=None, stream=None):
        """tetra_rx_handover_channels_device: reset_channels, and every listed channel with a donor (donors[i] >= 0; -1: a plain restart)
        inherits that channel's frame timing, cell and TDMA clock and looks for its first burst `window` bits either side of where the
        donor's frames start, for at most `max_slots` slot periods (None: the header's defaults).  Enqueued, not waited for."""
        ch = np.ascontiguousarray(np.asarray(channels, np.int64).astype(np.int32).reshape(-1))
        dn = np.ascontiguousarray(np.asarray(donors, np.int64).astype(np.int32).reshape(-1))
        if dn.size != ch.size:
            raise ValueError("handover_channels takes a donor (or -1) per channel")
        call(self._lib.tetra_rx_handover_channels_device, self._h, ptr(ch) if ch.size else None, ptr(dn) if dn.size else None, int(ch.size),
             handover_params_arg(window, max_slots), stream_ptr(stream))

    def resume(self, elapsed_bits, channels=None, window=None, max_slots=None, stream=None):
        """tetra_rx_resume_channels_device (include/ext/tetra_gap.h): the listed channels (None: all) restart as reset_channels restarts
        them, after `elapsed_bits` bits that never arrived, and a channel that was locked keeps its scrambling code, its TDMA clock
        advanced by the slots that passed, and looks for its first burst `window` bits either side of where its own frame grid puts it.
        handover_status() says what became of each.  Enqueued, not waited for."""
        ch = np.arange(self.n_channels, dtype=np.int32) if channels is None else np.ascontiguousarray(np.asarray(channels, np.int64).astype(np.int32).reshape(-1))
        call(self._lib.tetra_rx_resume_channels_device, self._h, ptr(ch) if ch.size else None, int(ch.size), int(elapsed_bits),
             gap_params_arg(window, max_slots), stream_ptr(stream))

    def handover_status(self, first=0, count=None):
        """tetra_rx_get_handover: per channel (state HANDOVER_*, slot periods waited, found - expected frame start in bits)."""
        return [(a.state, a.slots_waited, a.offset) for a in self._channel_table(self._lib.tetra_rx_get_handover, HandoverStatus, first, count)]

    def process(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        n = iq.size // self.n_channels
        call(self._lib.tetra_rx_process, self._h, ptr(iq), int(n))

    def process_device(self, d_iq, n_samples, stream=None):
        call(self._lib.tetra_rx_process_device, self._h, ptr(d_iq), int(n_samples), stream_ptr(stream))

    def wait(self):
        call(self._lib.tetra_rx_wait, self._h)

    def count(self, kind, which=0):
        n = C.c_int(0)
        call(self._lib.tetra_rx_fetch, self._h, which, kind, None, None, 0, 0, C.byref(n))
        return n.value

    def fetch(self, kind, which=0):
        """-> (blocks: structured array [n] of BLOCK_DTYPE, type1: uint8 [n][type1_bits(kind)])"""
        n = self.count(kind, which)
        nb = type1_bits(kind)
        blocks = np.zeros(max(n, 1), BLOCK_DTYPE)
        t1 = np.zeros((max(n, 1), nb), np.uint8)
        got = C.c_int(0)
        call(self._lib.tetra_rx_fetch, self._h, which, kind, ptr(blocks), ptr(t1), nb, max(n, 1), C.byref(got))
        return blocks[:got.value], t1[:got.value]

    def _count_then_fetch(self, fn, dtype, which, *kind):
        """A fetch entry point of the form fn(h, which, [kind,] out, capacity, &n_rows): asked for the row count, then for the rows."""
        n = C.c_int(0)
        call(fn, self._h, which, *kind, None, 0, C.byref(n))
        v = np.zeros(max(n.value, 1), dtype)
        got = C.c_int(0)
        call(fn, self._h, which, *kind, ptr(v), max(n.value, 1), C.byref(got))
        return v[:got.value]

    def fetch_aach_dist(self, which=0):
        """tetra_rx_fetch_aach_dist: uint8 [n], byte 30 of every BBK row in fetch(KIND_BBK)'s order -- the Hamming distance 0..3 the
        RM(30,14) decoder corrected, or AACH_UNDECODABLE; with FLAG_AACH_SOFT the non-zero soft values that disagree with the
        maximum-likelihood codeword.  Needs a handle created with FLAG_AACH_RM3014 or FLAG_AACH_SOFT."""
        return self._count_then_fetch(self._lib.tetra_rx_fetch_aach_dist, np.uint8, which)

    def set_aach_min_margin(self, min_margin):
        """tetra_rx_set_aach_min_margin: the margin (1..930) from which the calls that follow accept a maximum-likelihood AACH row.
        Needs a handle created with FLAG_AACH_SOFT."""
        call(self._lib.tetra_rx_set_aach_min_margin, self._h, int(min_margin))

    def fetch_aach_margin(self, which=0):
        """tetra_rx_fetch_aach_margin: uint16 [n], byte 31 of every BBK row in fetch(KIND_BBK)'s order -- the margin of the
        maximum-likelihood codeword to the runner-up, saturated at 255 (0: a tie).  Needs a handle created with FLAG_AACH_SOFT."""
        return self._count_then_fetch(self._lib.tetra_rx_fetch_aach_margin, np.uint16, which)

    def fetch_biterr(self, kind, which=0):
        """tetra_rx_fetch_biterr: (errors, compared) int arrays [n] of a coded kind's rows, in fetch(kind)'s order -- the distance from
        the received block to the decoded codeword and the positions it was taken over; an estimate of the channel's bit errors that
        is meaningful for rows with a good CRC.  Needs a handle created with FLAG_BITERR."""
        v = self._count_then_fetch(self._lib.tetra_rx_fetch_biterr, np.uint32, which, kind).astype(np.int64)
        return v & 0xffff, v >> 16

    def biterr_device(self, kind, which=0, stream=None):
        """tetra_rx_biterr_device -> the raw device address of the kind's counts (uint32 per row of rows_device)."""
        return self._column_device(self._lib.tetra_rx_biterr_device, kind, which, stream)

    def _column_device(self, fn, kind, which, stream):
        """A device view of the form fn(h, which, kind, &d_column, stream) -> the raw device address."""
        d = C.c_void_p()
        call(fn, self._h, which, kind, C.byref(d), stream_ptr(stream))
        return d.value

    def set_list_candidates(self, max_candidates):
        """tetra_rx_set_list_candidates: how many next-best paths (1..8) the calls that follow try on a CRC-failed block.  Needs a handle
        created with FLAG_LIST."""
        call(self._lib.tetra_rx_set_list_candidates, self._h, int(max_candidates))

    def fetch_list_rank(self, kind, which=0):
        """tetra_rx_fetch_list_rank: int32 [n] of a coded kind's rows, in fetch(kind)'s order -- 0: the decoder's own path passed the CRC,
        k >= 1: rescued by candidate k, -1: failed and not rescued.  Needs a handle created with FLAG_LIST."""
        return self._count_then_fetch(self._lib.tetra_rx_fetch_list_rank, np.int32, which, kind)

    def list_rank_device(self, kind, which=0, stream=None):
        """tetra_rx_list_rank_device -> the raw device address of the kind's ranks (int32 per row of rows_device)."""
        return self._column_device(self._lib.tetra_rx_list_rank_device, kind, which, stream)

    def links(self, first=0, count=None):
        """tetra_rx_get_link: per channel a dict bits / bit_errors (summed over the coded blocks with a good CRC since the last reset)
        and blocks / blocks_crc_bad (every coded block)."""
        return [dict(bits=int(a.bits), bit_errors=int(a.bit_errors), blocks=int(a.blocks), blocks_crc_bad=int(a.blocks_crc_bad))
                for a in self._channel_table(self._lib.tetra_rx_get_link, Link, first, count)]

    def _channel_table(self, fn, elem, first, count):
        """A per-channel getter of the form fn(h, first, count, out) -> [elem] of channels first .. first + count - 1 (None: to the last)."""
        count = self.n_channels - first if count is None else count
        arr = (elem * max(count, 1))()
        call(fn, self._h, int(first), int(count), arr)
        return [arr[i] for i in range(count)]

    def cells(self, first=0, count=None):
        return self._channel_table(self._lib.tetra_rx_get_cell, CellState, first, count)

    def sync_states(self, first=0, count=None):
        return [(a.state, a.bits_in_buf, a.bitbuf_start_bitnum, a.next_frame_start_bitnum)
                for a in self._channel_table(self._lib.tetra_rx_get_sync_state, BsyncState, first, count)]

    def set_sync_tolerance(self, tol):
        """tetra_rx_set_sync_tolerance: (tol_norm, tol_sync, max_miss) for the synchroniser's tolerant lock from the next call on, None =
        the reference's rule.  Between process calls; waits for the tail in flight."""
        call(self._lib.tetra_rx_set_sync_tolerance, self._h, tolerance_arg(tol))

    def sync_misses(self, first=0, count=None):
        """tetra_rx_get_sync_misses: int32 [count], per channel the consecutive LOCKED frames without a training sequence."""
        return np.array(self._channel_table(self._lib.tetra_rx_get_sync_misses, C.c_int32, first, count), np.int32)

    def stage_ms(self):
        ms = (C.c_float * 4)()
        call(self._lib.tetra_rx_stage_ms, self._h, C.byref(ms))
        return [float(v) for v in ms]

    def rows_device(self, kind, which=0, stream=None):
        """-> (d_type2 pointer, type2_stride, d_blocks pointer, d_n_rows pointer): raw device addresses."""
        t2, blk, nr, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        call(self._lib.tetra_rx_rows_device, self._h, which, kind, C.byref(t2), C.byref(st), C.byref(blk), C.byref(nr), stream_ptr(stream))
        return t2.value, st.value, blk.value, nr.value

    def bits_device(self, which=0, stream=None):
        bits, nb, st = C.c_void_p(), C.c_void_p(), C.c_int(0)
        call(self._lib.tetra_rx_bits_device, self._h, which, C.byref(bits), C.byref(st), C.byref(nb), stream_ptr(stream))
        return bits.value, st.value, nb.value

    def demod_handle(self):
        return self._lib.tetra_rx_demod(self._h)

    # ---- include/ext/tetra_traffic.h ----
    def enable_traffic(self, max_rows=None):
        """tetra_rx_traffic_enable: once per handle, synchronises; max_rows (None: the handle's max_rows) rows per TCH kind and call are
        kept.  Until then every traffic method raises TETRA_ERR_UNSUPPORTED."""
        call(self._lib.tetra_rx_traffic_enable, self._h, int(self.max_rows if max_rows is None else max_rows))

    def set_traffic(self, table, first=0, stream=None):
        """tetra_rx_set_traffic: the entries of channels first .. first + len(table) - 1 (traffic_table_arg: per channel {tn: kind} or
        {tn: (kind, usage)}, or a TRAFFIC_SLOT_DTYPE array [n][4]), from the next process call on; enqueued on `stream`, not waited for."""
        t = traffic_table_arg(table)
        call(self._lib.tetra_rx_set_traffic, self._h, int(first), int(t.shape[0]), ptr(t) if t.size else None, stream_ptr(stream))

    def traffic(self, first=0, count=None):
        """tetra_rx_get_traffic -> TRAFFIC_SLOT_DTYPE array [count][4], the table on the device."""
        count = self.n_channels - first if count is None else count
        t = np.zeros((max(count, 1), 4), TRAFFIC_SLOT_DTYPE)
        call(self._lib.tetra_rx_get_traffic, self._h, int(first), int(count), ptr(t))
        return t[:count]

    def fetch_traffic(self, tch_kind, which=0, biterr=False):
        """tetra_rx_fetch_traffic -> (blocks [n] of BLOCK_DTYPE, type2 uint8 [n][TRAFFIC_TYPE2_BITS[tch_kind]], rows dropped beyond
        max_rows) and, with biterr (FLAG_BITERR, the coded kinds), the uint32 words errors | compared << 16 [n] as a fourth."""
        n, dropped = C.c_int(0), C.c_int(0)
        call(self._lib.tetra_rx_fetch_traffic, self._h, which, int(tch_kind), None, None, 0, 0, None, C.byref(n), C.byref(dropped))
        cap, nb = max(n.value, 1), TRAFFIC_TYPE2_BITS[int(tch_kind)]
        blocks, t2, be = np.zeros(cap, BLOCK_DTYPE), np.zeros((cap, nb), np.uint8), np.zeros(cap, np.uint32)
        call(self._lib.tetra_rx_fetch_traffic, self._h, which, int(tch_kind), ptr(blocks), ptr(t2), nb, cap, ptr(be) if biterr else None, C.byref(n),
             C.byref(dropped))
        out = (blocks[:n.value], t2[:n.value], dropped.value)
        return out + (be[:n.value],) if biterr else out

    def traffic_rows_device(self, tch_kind, which=0, stream=None):
        """tetra_rx_traffic_rows_device -> (d_type2, type2_stride, d_blocks, d_counts [routed, kept, dropped], d_biterr or None): raw
        device addresses."""
        t2, blk, cnt, be, st = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(0)
        call(self._lib.tetra_rx_traffic_rows_device, self._h, which, int(tch_kind), C.byref(t2), C.byref(st), C.byref(blk), C.byref(cnt), C.byref(be),
             stream_ptr(stream))
        return t2.value, st.value, blk.value, cnt.value, be.value

    def set_snapshot(self, chan_extras):
        """tetra_rx_out_set_snapshot: the channel extras (EXT_CHAN_*) every tail from the next call on copies into its call's snapshot,
        which deliver(extras=...) of that call then reads; 0 disarms."""
        call(self._lib.tetra_rx_out_set_snapshot, self._h, int(chan_extras))

    def deliver(self, which=0, kinds=0, packed=False, crc_good_only=False, buf=None, extras=0):
        """Enqueue a delivery of the latest (which = 0) or previous (1) call's blocks of `kinds` (bit mask, 0 = every configured kind)
        and return a Delivery without waiting.  buf = None: the next of two page-locked buffers of this handle (sized for the worst case),
        so the arrays a Delivery returns stay valid until the second delivery after it is enqueued; else a HostBuffer, a torch tensor on
        the handle's GPU, or any object with a .ctypes pointer (pageable memory is refused: TETRA_ERR_ARG).
        extras (EXT_ROW_* | EXT_CHAN_*, include/ext/tetra_rx_out_ext.h): the rows' opt-in columns and the call's per-channel state in
        the same buffer; the channel extras need set_snapshot armed with them when that call was processed."""
        flags = (OUT_PACKED if packed else 0) | (OUT_CRC_GOOD if crc_good_only else 0)
        if buf is None:
            if getattr(self, "_pool", None) is None:
                # sized once, for every extra this handle can ever deliver (the miss counters may be enabled later: counted by hand)
                nb, can = C.c_uint64(0), 0
                for _, bit, _ in ROW_COLUMNS + CHAN_TABLES:
                    if bit != EXT_CHAN_SYNC_MISSES and self._lib.tetra_rx_out_bound_ext(self._h, 0, 0, bit, C.byref(nb)) == 0:
                        can |= bit
                call(self._lib.tetra_rx_out_bound_ext, self._h, 0, 0, can, C.byref(nb))
                misses = next(dtype for _, bit, dtype in CHAN_TABLES if bit == EXT_CHAN_SYNC_MISSES)
                self._pool, self._pool_next = [HostBuffer(nb.value + 16 + misses.itemsize * self.n_channels) for _ in range(2)], 0
            buf = self._pool[self._pool_next]
            self._pool_next ^= 1
        if isinstance(buf, HostBuffer):
            dst, cap = buf.ptr, buf.nbytes
        elif hasattr(buf, "data_ptr"):
            dst, cap = buf.data_ptr(), buf.numel() * buf.element_size()
        else:
            dst, cap = buf.ctypes.data, buf.nbytes
        ticket = C.c_int64(-1)
        if extras:
            call(self._lib.tetra_rx_out_enqueue_ext, self._h, which, kinds, flags, int(extras), dst, cap, C.byref(ticket))
        else:
            call(self._lib.tetra_rx_out_enqueue, self._h, which, kinds, flags, dst, cap, C.byref(ticket))
        return Delivery(self, ticket.value, buf, cap, extras)

    def out_bound(self, kinds=0, packed=False, crc_good_only=False, extras=0):
        nb = C.c_uint64(0)
        flags = (OUT_PACKED if packed else 0) | (OUT_CRC_GOOD if crc_good_only else 0)
        if extras:
            call(_lib().tetra_rx_out_bound_ext, self._h, kinds, flags, int(extras), C.byref(nb))
        else:
            call(_lib().tetra_rx_out_bound, self._h, kinds, flags, C.byref(nb))
        return nb.value

    def _close_pool(self):
        for b in getattr(self, "_pool", None) or []:
            b.close()
        self._pool = None


# ---- one-step hand-off of a call's blocks (include/tetra_rx_out.h) ----

OUT_PACKED, OUT_CRC_GOOD = 1, 2
OUT_MAGIC = 0x4f585254


class OutKind(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_rows", C.c_int32), ("n_rows_decoded", C.c_int32), ("row_bytes", C.c_int32),
                ("blocks_offset", C.c_uint64), ("bits_offset", C.c_uint64)]


class OutHeader(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("status", C.c_int32), ("flags", C.c_int32), ("n_kinds", C.c_int32), ("call", C.c_int64),
                ("bytes", C.c_uint64), ("kinds", OutKind * N_KINDS)]


# the extension block (include/ext/tetra_rx_out_ext.h)
EXT_ROW_BITERR, EXT_ROW_LIST_RANK, EXT_ROW_AACH_DIST = 1, 2, 4
EXT_CHAN_CELL, EXT_CHAN_SYNC_STATE, EXT_CHAN_SYNC_MISSES, EXT_CHAN_LINK = 16, 32, 64, 128
EXT_ROW_ALL, EXT_CHAN_ALL = 7, 240
OUT_EXT_MAGIC = 0x58585254
CELL_DTYPE = np.dtype([(n, "<u4") for n, _ in CellState._fields_])
SYNC_STATE_DTYPE = np.dtype([("state", "<i4"), ("bits_in_buf", "<u4"), ("bitbuf_start_bitnum", "<u4"), ("next_frame_start_bitnum", "<u4")])
LINK_DTYPE = np.dtype([("bits", "<u8"), ("bit_errors", "<u8"), ("blocks", "<u4"), ("blocks_crc_bad", "<u4")])
# The extension block's row columns and per-channel tables, in its order, as (name, EXT_* bit, element dtype): what view_delivery_ext
# returns under these names, what DeliveryRows documents, and what RxChain.deliver sizes its pool for.
ROW_COLUMNS = (("biterr", EXT_ROW_BITERR, np.dtype("<u4")), ("rank", EXT_ROW_LIST_RANK, np.dtype("<i4")), ("aach_dist", EXT_ROW_AACH_DIST, np.dtype("u1")))
CHAN_TABLES = (("cell", EXT_CHAN_CELL, CELL_DTYPE), ("sync_state", EXT_CHAN_SYNC_STATE, SYNC_STATE_DTYPE),
               ("sync_misses", EXT_CHAN_SYNC_MISSES, np.dtype("<i4")), ("link", EXT_CHAN_LINK, LINK_DTYPE))


class OutExtKind(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_rows", C.c_int32)] + [(name + "_offset", C.c_uint64) for name, _, _ in ROW_COLUMNS]


class OutExtHeader(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("extras", C.c_int32), ("call", C.c_int64), ("n_channels", C.c_int32), ("n_kinds", C.c_int32),
                ("bytes", C.c_uint64)] + [(name + "_offset", C.c_uint64) for name, _, _ in CHAN_TABLES] + [("kinds", OutExtKind * N_KINDS)]


class HostBuffer:
    """Page-locked, coherent host memory mapped for the GPUs (tetra_rx_out_host_alloc); .array is a uint8 numpy view of it."""

    def __init__(self, nbytes):
        self._lib = _lib()
        self.nbytes = int(nbytes)
        self.ptr = self._lib.tetra_rx_out_host_alloc(self.nbytes)
        if not self.ptr:
            check(-5, self._lib.tetra_rx_out_host_alloc)
        self.array = np.ctypeslib.as_array((C.c_uint8 * self.nbytes).from_address(self.ptr))

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._lib.tetra_rx_out_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _open_delivery(buf, nbytes):
    """-> (library, uint8 array, its bytes, its address, classic header) of a delivery in host memory"""
    arr = buf.array if isinstance(buf, HostBuffer) else buf
    return _lib(), arr, arr.nbytes if nbytes is None else int(nbytes), arr.ctypes.data, OutHeader.from_buffer_copy(arr[:C.sizeof(OutHeader)].tobytes())


def view_delivery(buf, nbytes=None):
    """A completed delivery in host memory (numpy uint8 array, or HostBuffer) -> (header, {kind: (blocks, type1)}): numpy views into
    the buffer; type1 is [n][row_bytes] (packed rows when the header's flags say so).  A header status other than TETRA_OK raises."""
    L, arr, nbytes, base, hd = _open_delivery(buf, nbytes)
    out = {}
    for i in range(max(0, min(hd.n_kinds, N_KINDS))):
        k = hd.kinds[i].kind
        pb, pt, n, rb = C.c_void_p(), C.c_void_p(), C.c_int(0), C.c_int(0)
        call(L.tetra_rx_out_view, base, nbytes, k, C.byref(pb), C.byref(pt), C.byref(n), C.byref(rb))
        ob, ot = pb.value - base, pt.value - base
        blocks = arr[ob: ob + n.value * BLOCK_DTYPE.itemsize].view(BLOCK_DTYPE)
        out[k] = (blocks, arr[ot: ot + n.value * rb.value].reshape(n.value, rb.value))
    return hd, out


def view_delivery_ext(buf, nbytes=None):
    """The extension block of a completed extended delivery in host memory -> (extension header, {kind: {column: [n] or None}} for the
    columns of ROW_COLUMNS, {table: [C] or None} for the tables of CHAN_TABLES, each with the dtype given there and None where the
    delivery does not hold it): numpy views into the buffer (tetra_rx_out_view_ext / tetra_rx_out_view_channels).  A buffer without an
    extension block raises (TETRA_ERR_UNSUPPORTED)."""
    L, arr, nbytes, base, hd = _open_delivery(buf, nbytes)

    def at(p, n, dtype):
        if not p.value:
            return None
        o = p.value - base
        return arr[o: o + n * dtype.itemsize].view(dtype)

    cols = {}
    for i in range(max(0, min(hd.n_kinds, N_KINDS))):
        k = hd.kinds[i].kind
        ps, n = [C.c_void_p() for _ in ROW_COLUMNS], C.c_int(0)
        call(L.tetra_rx_out_view_ext, base, nbytes, k, *[C.byref(p) for p in ps], C.byref(n))
        cols[k] = {name: at(p, n.value, dtype) for (name, _, dtype), p in zip(ROW_COLUMNS, ps)}
    ps, nc = [C.c_void_p() for _ in CHAN_TABLES], C.c_int(0)
    call(L.tetra_rx_out_view_channels, base, nbytes, *[C.byref(p) for p in ps], C.byref(nc))
    chans = {name: at(p, nc.value, dtype) for (name, _, dtype), p in zip(CHAN_TABLES, ps)}
    o = (int(hd.bytes) + 15) // 16 * 16
    return OutExtHeader.from_buffer_copy(arr[o: o + C.sizeof(OutExtHeader)].tobytes()), cols, chans


class DeliveryRows(dict):
    __doc__ = ("""What Delivery.wait() returns: {kind: (blocks, type1)}, and for an extended delivery .columns = {kind: {%s}} and
    .channels = {%s} (view_delivery_ext); both None otherwise.""" %
               tuple(", ".join('"%s"' % name for name, _, _ in t) for t in (ROW_COLUMNS, CHAN_TABLES)))
    columns = None
    channels = None


def unpack_bits(packed, n_bits):
    """Packed rows [n][row_bytes] (first bit in bit 7) -> uint8 [n][n_bits], one bit per byte (tetra_rx_unpack_bits)."""
    packed = np.ascontiguousarray(packed, np.uint8)
    n, rb = packed.shape
    out = np.zeros((n, n_bits), np.uint8)
    call(_lib().tetra_rx_unpack_bits, ptr(packed), n, rb, n_bits, ptr(out), n_bits)
    return out


def out_rows_workspace_bytes(max_rows):
    """tetra_rx_out_rows_workspace_bytes: device scratch for out_write_rows over up to max_rows rows per kind."""
    return int(_lib().tetra_rx_out_rows_workspace_bytes(int(max_rows)))


def out_rows_arg(kinds):
    """[dict(kind, type2, crc_ok, blocks, n_rows[, stride, biterr, rank])] -> the tetra_rx_out_rows_t array.  Every array is a torch
    tensor on the GPU or a raw device address (ptr's rule); stride defaults to type2's row length in bytes, which a raw address lacks."""
    arr = (OutRows * max(len(kinds), 1))()
    for o, k in zip(arr, kinds):
        t2 = k["type2"]
        stride = k.get("stride")
        o.kind, o.type2_stride = int(k["kind"]), int(t2.stride(0) * t2.element_size() if stride is None else stride)
        o.d_type2, o.d_crc_ok, o.d_blocks, o.d_n_rows = ptr(t2), ptr(k["crc_ok"]), ptr(k["blocks"]), ptr(k["n_rows"])
        o.d_biterr, o.d_rank = ptr(k.get("biterr")), ptr(k.get("rank"))
    return arr


def out_write_rows(kinds, max_rows, dst, workspace, packed=False, crc_good_only=False, row_extras=0, call_index=0, capacity=None, stream=None):
    """tetra_rx_out_write_rows_device (include/ext/tetra_rx_out_rows.h): the delivery's launches over the caller's rows `kinds`
    (out_rows_arg's list, ascending kinds), enqueued on `stream` and not waited for.  dst: a HostBuffer, a uint8 torch tensor on the
    GPU or an object with a .ctypes pointer into page-locked memory (capacity: its size unless given); workspace: a uint8 torch tensor of out_rows_workspace_bytes(max_rows) bytes on the GPU.  Read
    the result with view_delivery / view_delivery_ext once the stream's work is done."""
    flags = (OUT_PACKED if packed else 0) | (OUT_CRC_GOOD if crc_good_only else 0)
    if isinstance(dst, HostBuffer):
        d, cap = dst.ptr, dst.nbytes
    elif hasattr(dst, "data_ptr"):
        d, cap = dst.data_ptr(), dst.numel() * dst.element_size()
    else:
        d, cap = dst.ctypes.data, dst.nbytes
    call(_lib().tetra_rx_out_write_rows_device, out_rows_arg(kinds), len(kinds), int(max_rows), flags, int(row_extras), int(call_index), d,
         cap if capacity is None else int(capacity), ptr(workspace), workspace.numel() * workspace.element_size(), stream_ptr(stream))


class Delivery:
    """One enqueued delivery (RxChain.deliver).  ready() polls; wait() blocks and returns {kind: (blocks, type1)}."""

    def __init__(self, chain, call, buf, capacity, extras=0):
        self.chain, self.call, self.buf, self.capacity, self.extras = chain, call, buf, capacity, extras
        self.header = self.ext_header = None

    def ready(self):
        rc = self.chain._lib.tetra_rx_out_query(self.chain._h, self.call)
        if rc < 0:
            check(rc, self.chain._lib.tetra_rx_out_query)
        return rc == 0

    def wait(self):
        call(self.chain._lib.tetra_rx_out_wait, self.chain._h, self.call)
        buf = self.buf
        if hasattr(buf, "data_ptr"):              # a device tensor: the header says how much to bring over
            head = buf[:C.sizeof(OutHeader)].cpu().numpy()
            hd = OutHeader.from_buffer_copy(head.tobytes())
            need = int(hd.bytes)
            if self.extras and hd.status == 0:      # the extension header behind the classic part says how long the whole is
                o = (need + 15) // 16 * 16
                if o + C.sizeof(OutExtHeader) <= self.capacity:
                    ex = OutExtHeader.from_buffer_copy(buf[o: o + C.sizeof(OutExtHeader)].cpu().numpy().tobytes())
                    need = int(ex.bytes) if ex.magic == OUT_EXT_MAGIC else need
            buf = buf[:min(need, self.capacity)].cpu().numpy() if need <= self.capacity else head
            self.host_copy = buf
        arr = buf.array if isinstance(buf, HostBuffer) else buf
        self.header = OutHeader.from_buffer_copy(arr[:C.sizeof(OutHeader)].tobytes())
        if self.header.status:
            raise TetraDemodError(self.header.status, "tetra_rx delivery (needs %d bytes)" % self.header.bytes)
        rows = DeliveryRows(view_delivery(buf, min(arr.nbytes, self.capacity))[1])
        if self.extras:
            self.ext_header, rows.columns, rows.channels = view_delivery_ext(buf, min(arr.nbytes, self.capacity))
        return rows

