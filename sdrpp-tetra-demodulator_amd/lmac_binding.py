"""ctypes binding of the batched lower-MAC channel decoding (include/tetra_lmac.h)."""
import ctypes as C
import functools

import numpy as np

from ._ffi import P, call, declare, i32, ptr, size_t, stream_ptr, u32, vp
from .binding import load_library

JOB_RM3014 = 0x100            # TETRA_LMAC_JOB_RM3014: OR into a BBK job's type for decode_frames_device
AACH_UNDECODABLE = 0xFF       # TETRA_AACH_UNDECODABLE
JOB_RM3014_SOFT = 0x200       # TETRA_LMAC_JOB_RM3014_SOFT: OR into a BBK job's type for decode_frames_soft (include/ext/tetra_aach_soft.h)
AACH_SOFT_MAX_MARGIN = 930    # TETRA_AACH_SOFT_MAX_MARGIN
# enum tp_sap_data_type (src/decoder/src/phy/tetra_burst.h:9-16)
TPSAP_T_SB1, TPSAP_T_SB2, TPSAP_T_NDB, TPSAP_T_BBK, TPSAP_T_SCH_HU, TPSAP_T_SCH_F = range(6)


class Label(C.Structure):
    """tetra_lmac_label_t (= tetra_rx_block_t)."""
    _fields_ = [("channel", C.c_int32), ("frame_slot", C.c_int32), ("bitnum", C.c_uint32), ("tdma_time_rx", C.c_uint32),
                ("tdma_time", C.c_uint32), ("crc_ok", C.c_int32)]


class Frames(C.Structure):
    """tetra_lmac_frames_t."""
    _fields_ = [("d_frames", C.c_void_p), ("d_frame_type", C.c_void_p), ("n_frames", C.c_int32), ("frames_per_channel", C.c_int32),
                ("d_frame_bitnum", C.c_void_p), ("d_time_rx", C.c_void_p), ("d_time", C.c_void_p), ("d_workspace", C.c_void_p),
                ("workspace_bytes", C.c_size_t)]


class Job(C.Structure):
    """tetra_lmac_job_t."""
    _fields_ = [("type", C.c_int32), ("blk_num", C.c_int32), ("d_row_frame", C.c_void_p), ("d_n_rows", C.c_void_p), ("max_rows", C.c_int32),
                ("out_stride", C.c_int32), ("d_frame_scramb", C.c_void_p), ("d_type2", C.c_void_p), ("d_crc_ok", C.c_void_p),
                ("d_labels", C.c_void_p)]


class BlkParam(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("type345_bits", "type2_bits", "type1_bits", "interleave_a", "have_crc16")]


# include/tetra_lmac.h
SIGNATURES = {
    "tetra_lmac_blk_param": (i32, [i32, P(BlkParam)]),
    "tetra_lmac_scramb_init": (u32, [C.c_uint16, C.c_uint16, C.c_uint8]),
    "tetra_lmac_decode_batch_device": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, vp]),
    "tetra_lmac_decode_counted_device": (i32, [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp]),
    "tetra_lmac_debug_force_byte_route": (i32, [i32]),
    "tetra_lmac_decode_frames_device": (i32, [P(Frames), P(Job), i32, vp]),
    "tetra_lmac_decode_frames_workspace_bytes": (size_t, [P(Job), i32]),
    "tetra_lmac_decode_batch": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32]),
    "tetra_lmac_track_scramb_device": (i32, [vp, i32, vp, vp, i32, i32, vp, vp, vp]),
    "tetra_lmac_track_sync_device": (i32, [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "tetra_lmac_track_sync_lists_device": (i32, [vp, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
}
# include/tetra_aach.h: the lower MAC's share (the receive chain's is in rx_binding.AACH_SIGNATURES)
AACH_SIGNATURES = {
    "tetra_lmac_rm3014_decode_device": (i32, [vp, i32, vp, vp, vp]),
    "tetra_lmac_decode_aach_rm3014_device": (i32, [vp, i32, i32, vp, vp, i32, vp, vp]),
}
# include/ext/tetra_biterr.h: the lower MAC's share (the receive chain's is in rx_binding.BITERR_ABI)
BITERR_ABI = {
    "tetra_lmac_decode_counted_biterr_device": (i32, [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp]),
    "tetra_lmac_decode_batch_biterr": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, vp, i32]),
    "tetra_lmac_decode_frames_biterr_device": (i32, [P(Frames), P(Job), i32, P(vp), vp]),
}
# include/ext/tetra_list.h: the lower MAC's share
LIST_ABI = {
    "tetra_lmac_decode_counted_list_device": (i32, [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, vp, vp]),
    "tetra_lmac_decode_batch_list": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32, vp, i32]),
    "tetra_lmac_decode_frames_list_device": (i32, [P(Frames), P(Job), i32, i32, P(vp), vp]),
}
LIST_MAX_CANDIDATES, LIST_DEFAULT_CANDIDATES = 8, 4            # TETRA_LIST_MAX_CANDIDATES, TETRA_LIST_DEFAULT_CANDIDATES
# include/ext/tetra_soft.h
SOFT_ABI = {
    "tetra_lmac_decode_frames_soft_device": (i32, [P(Frames), P(Job), i32, vp, u32, P(vp), P(vp), i32, vp]),
}
# include/ext/tetra_aach_soft.h: the lower MAC's share (the receive chain's is in rx_binding.AACH_SOFT_ABI)
AACH_SOFT_ABI = {
    "tetra_lmac_rm3014_soft_decode_device": (i32, [vp, i32, i32, vp, vp, vp, vp]),
}
# include/ext/tetra_tch.h: the circuit-mode data channels; the kinds go where a TPSAP_T_* goes in decode_frames_device's job list
TCH_ABI = {
    "tetra_lmac_tch_blk_param": (i32, [i32, P(BlkParam)]),
    "tetra_lmac_decode_tch_counted_device": (i32, [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp]),
    "tetra_lmac_decode_tch_batch": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32]),
}
T_TCH_7_2, T_TCH_4_8, T_TCH_2_4 = 8, 9, 10          # TETRA_LMAC_T_TCH_*
# include/ext/tetra_tch_soft.h: TCH/4.8 and TCH/2.4 from soft values
TCH_SOFT_ABI = {
    "tetra_lmac_decode_tch_soft_counted_device": (i32, [i32, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp]),
    "tetra_lmac_decode_tch_soft_batch": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32]),
    "tetra_lmac_decode_frames_soft_tch_device": (i32, [P(Frames), P(Job), i32, vp, u32, P(vp), P(vp), i32, vp]),
}
# include/ext/tetra_tch_nblk.h: TCH/4.8 and TCH/2.4 interleaved over N = 1, 4 or 8 blocks, hard bits and soft values
TCH_NBLK_ABI = {
    "tetra_lmac_decode_tch_nblk_device": (i32, [i32, i32, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]),
    "tetra_lmac_decode_tch_nblk_soft_device": (i32, [i32, i32, vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]),
    "tetra_lmac_decode_tch_nblk_batch": (i32, [i32, i32, vp, i32, i32, vp, vp, i32, vp, i32, vp, i32]),
    "tetra_lmac_decode_tch_nblk_soft_batch": (i32, [i32, i32, vp, i32, i32, vp, vp, i32, vp, i32, vp, i32]),
}
LMAC_EXPORTS, AACH_EXPORTS, BITERR_EXPORTS, LIST_EXPORTS = list(SIGNATURES), list(AACH_SIGNATURES), list(BITERR_ABI), list(LIST_ABI)
SOFT_EXPORTS = list(SOFT_ABI)
AACH_SOFT_EXPORTS = list(AACH_SOFT_ABI)
TCH_EXPORTS = list(TCH_ABI)
TCH_SOFT_EXPORTS = list(TCH_SOFT_ABI)
TCH_NBLK_EXPORTS = list(TCH_NBLK_ABI)


@functools.lru_cache(None)
def _lib():
    # (a TETRA_DEMOD_LIB override may be an older build without the Reed-Muller decoder)
    return declare(load_library(), {**SIGNATURES, **AACH_SIGNATURES, **BITERR_ABI, **LIST_ABI, **SOFT_ABI, **AACH_SOFT_ABI, **TCH_ABI, **TCH_SOFT_ABI,
                                     **TCH_NBLK_ABI},
                   optional=AACH_EXPORTS + BITERR_EXPORTS + LIST_EXPORTS + SOFT_EXPORTS + AACH_SOFT_EXPORTS + TCH_EXPORTS + TCH_SOFT_EXPORTS +
                   TCH_NBLK_EXPORTS)


def force_byte_route(on):
    """tetra_lmac_debug_force_byte_route: every row through the decoder's byte route (process-wide).  Returns the old setting."""
    return bool(_lib().tetra_lmac_debug_force_byte_route(int(bool(on))))


def blk_param(blk_type):
    p = BlkParam()
    call(_lib().tetra_lmac_blk_param, int(blk_type), C.byref(p))
    return p


def scramb_init(mcc, mnc, colour):
    return int(_lib().tetra_lmac_scramb_init(int(mcc) & 0xffff, int(mnc) & 0xffff, int(colour) & 0xff))


def out_stride_for(blk_type):
    return (blk_param(blk_type).type2_bits + 3) & ~3


def _host_batch(blk_type, type5, scramb):
    """What every decode_batch* call hands over: the rows, their count and stride, the scrambling codes, the output rows with their
    stride, and the verdicts."""
    rows = np.ascontiguousarray(type5, np.uint8)
    n, in_stride = rows.shape
    ost = out_stride_for(blk_type)
    si = None if scramb is None else np.ascontiguousarray(scramb, np.uint32)
    return rows, n, in_stride, si, np.zeros((n, ost), np.uint8), ost, np.zeros(n, np.int32)


def decode_batch(blk_type, type5, scramb=None, device=-1):
    """type5 uint8 [n][in_stride] (in_stride % 4 == 0), scramb uint32 [n] (None for SB1)
    -> (type2 uint8 [n][type2_bits rounded up to 4], crc_ok int32 [n])."""
    rows, n, in_stride, si, out, ost, ok = _host_batch(blk_type, type5, scramb)
    call(_lib().tetra_lmac_decode_batch, int(blk_type), ptr(rows), n, in_stride, ptr(si), ptr(out), ost, ptr(ok), device)
    return out, ok


def decode_batch_device(blk_type, d_type5, n_blocks, in_stride, d_scramb, d_type2, out_stride, d_crc_ok, stream=None):
    """torch tensors already on the GPU; enqueues on `stream` (torch stream or raw handle), no synchronisation."""
    call(_lib().tetra_lmac_decode_batch_device, int(blk_type), ptr(d_type5), int(n_blocks), int(in_stride), ptr(d_scramb), ptr(d_type2),
         int(out_stride), ptr(d_crc_ok), stream_ptr(stream))


def decode_counted_device(blk_type, d_type5, capacity, d_n_blocks, in_stride, d_scramb, d_init_index, d_type2, out_stride, d_crc_ok,
                          stream=None):
    """Rows from the compacting demultiplexer: count and scrambling-code index are read on the device."""
    call(_lib().tetra_lmac_decode_counted_device, int(blk_type), ptr(d_type5), int(capacity), ptr(d_n_blocks), int(in_stride), ptr(d_scramb),
         ptr(d_init_index), ptr(d_type2), int(out_stride), ptr(d_crc_ok), stream_ptr(stream))


def split_biterr(biterr):
    """errors | compared << 16 (include/ext/tetra_biterr.h) -> (errors, compared) as int arrays."""
    v = np.asarray(biterr).astype(np.int64) & 0xffffffff          # (an int32 view of the words included)
    return v & 0xffff, v >> 16


def decode_batch_biterr(blk_type, type5, scramb=None, device=-1):
    """tetra_lmac_decode_batch_biterr: decode_batch plus the channel bit-error counts -> (type2, crc_ok, biterr uint32 [n])."""
    rows, n, in_stride, si, out, ost, ok = _host_batch(blk_type, type5, scramb)
    be = np.zeros(n, np.uint32)
    call(_lib().tetra_lmac_decode_batch_biterr, int(blk_type), ptr(rows), n, in_stride, ptr(si), ptr(out), ost, ptr(ok), ptr(be), device)
    return out, ok, be


def decode_counted_biterr_device(blk_type, d_type5, capacity, d_n_blocks, in_stride, d_scramb, d_init_index, d_type2, out_stride, d_crc_ok,
                                 d_biterr, stream=None):
    """tetra_lmac_decode_counted_biterr_device: decode_counted_device plus d_biterr (int32 / uint32 tensor [capacity], or None)."""
    call(_lib().tetra_lmac_decode_counted_biterr_device, int(blk_type), ptr(d_type5), int(capacity), ptr(d_n_blocks), int(in_stride), ptr(d_scramb),
         ptr(d_init_index), ptr(d_type2), int(out_stride), ptr(d_crc_ok), ptr(d_biterr), stream_ptr(stream))


def tch_blk_param(kind):
    """tetra_lmac_tch_blk_param (include/ext/tetra_tch.h): the block parameters of T_TCH_7_2 / T_TCH_4_8 / T_TCH_2_4."""
    p = BlkParam()
    call(_lib().tetra_lmac_tch_blk_param, int(kind), C.byref(p))
    return p


def decode_tch(kind, type5, scramb_init, biterr=False, device=-1):
    """tetra_lmac_decode_tch_batch: type5 uint8 [n][in_stride] (in_stride % 4 == 0, >= 432), scramb_init uint32 [n]
    -> type2 uint8 [n][type2_bits], and with biterr=True also the channel bit-error words uint32 [n] (split_biterr; not for T_TCH_7_2)."""
    rows = np.ascontiguousarray(type5, np.uint8)
    n, in_stride = rows.shape
    ost = tch_blk_param(kind).type2_bits
    si = np.ascontiguousarray(scramb_init, np.uint32)
    out = np.zeros((n, ost), np.uint8)
    be = np.zeros(n, np.uint32) if biterr else None
    call(_lib().tetra_lmac_decode_tch_batch, int(kind), ptr(rows), n, in_stride, ptr(si), ptr(out), ost, ptr(be), device)
    return (out, be) if biterr else out


def decode_tch_counted_device(kind, d_type5, capacity, d_n_blocks, in_stride, d_scramb, d_init_index, d_type2, out_stride, d_biterr=None, stream=None):
    """tetra_lmac_decode_tch_counted_device: torch tensors on the GPU; d_n_blocks, d_init_index and d_biterr may be None."""
    call(_lib().tetra_lmac_decode_tch_counted_device, int(kind), ptr(d_type5), int(capacity), ptr(d_n_blocks), int(in_stride), ptr(d_scramb),
         ptr(d_init_index), ptr(d_type2), int(out_stride), ptr(d_biterr), stream_ptr(stream))


def decode_tch_soft(kind, soft5, scramb_init, biterr=False, device=-1):
    """tetra_lmac_decode_tch_soft_batch (include/ext/tetra_tch_soft.h): soft5 int8 [n][in_stride] (in_stride % 4 == 0, >= 432; positive =
    bit 0, |value| <= 31), scramb_init uint32 [n] -> type2 uint8 [n][type2_bits], and with biterr=True also the channel bit-error words
    uint32 [n] (split_biterr).  T_TCH_4_8 / T_TCH_2_4 only."""
    rows = np.ascontiguousarray(soft5, np.int8)
    n, in_stride = rows.shape
    ost = tch_blk_param(kind).type2_bits
    si = np.ascontiguousarray(scramb_init, np.uint32)
    out = np.zeros((n, ost), np.uint8)
    be = np.zeros(n, np.uint32) if biterr else None
    call(_lib().tetra_lmac_decode_tch_soft_batch, int(kind), ptr(rows), n, in_stride, ptr(si), ptr(out), ost, ptr(be), device)
    return (out, be) if biterr else out


def decode_tch_soft_counted_device(kind, d_soft, capacity, d_n_blocks, in_stride, d_scramb, d_init_index, d_type2, out_stride, d_biterr=None, stream=None):
    """tetra_lmac_decode_tch_soft_counted_device: torch tensors on the GPU (d_soft int8); d_n_blocks, d_init_index and d_biterr may be None."""
    call(_lib().tetra_lmac_decode_tch_soft_counted_device, int(kind), ptr(d_soft), int(capacity), ptr(d_n_blocks), int(in_stride), ptr(d_scramb),
         ptr(d_init_index), ptr(d_type2), int(out_stride), ptr(d_biterr), stream_ptr(stream))


def tch_windows(stream_lengths, n, lost=()):
    """The sliding-window table of include/ext/tetra_tch_nblk.h for streams laid end to end in the pool: a stream of L received rows gives
    L - n + 1 output blocks (none if L < n), block b of it the rows b .. b + n - 1 of the stream; every listed pool row in `lost` is marked -1.
    -> int32 [n_blocks][n].  Pure: needs no library."""
    n = int(n)
    if n not in (1, 4, 8):
        raise ValueError("n must be 1, 4 or 8")
    rows, at = [], 0
    for length in stream_lengths:
        length = int(length)
        if length < 0:
            raise ValueError("a stream length is negative")
        rows += [np.arange(at + b, at + b + n) for b in range(length - n + 1)]
        at += length
    w = np.array(rows, np.int32).reshape(-1, n)
    gone = np.asarray(list(lost), np.int64)
    w[np.isin(w, gone)] = -1
    return w


def decode_tch_nblk(kind, n, rows, windows, scramb_init, soft=False, biterr=False, device=-1):
    """tetra_lmac_decode_tch_nblk_batch / _soft_batch (include/ext/tetra_tch_nblk.h): rows uint8 (soft: int8) [n_rows][in_stride], the pool
    of received bursts (in_stride % 4 == 0, >= 432); windows int32 [n_blocks][n] (tch_windows; an entry outside the pool = a lost burst);
    scramb_init uint32 [n_rows] -> type2 uint8 [n_blocks][type2_bits], and with biterr=True also the channel bit-error words uint32
    [n_blocks] (split_biterr).  T_TCH_4_8 / T_TCH_2_4, n in (1, 4, 8)."""
    pool = np.ascontiguousarray(rows, np.int8 if soft else np.uint8)
    n_rows, in_stride = pool.shape
    win = np.ascontiguousarray(windows, np.int32)
    if win.ndim != 2 or win.shape[1] != int(n):
        raise ValueError("windows must be [n_blocks][n]")
    ost = tch_blk_param(kind).type2_bits
    si = np.ascontiguousarray(scramb_init, np.uint32)
    if len(si) != n_rows:
        raise ValueError("scramb_init must have a code per pool row")
    out = np.zeros((len(win), ost), np.uint8)
    be = np.zeros(len(win), np.uint32) if biterr else None
    fn = _lib().tetra_lmac_decode_tch_nblk_soft_batch if soft else _lib().tetra_lmac_decode_tch_nblk_batch
    call(fn, int(kind), int(n), ptr(pool), n_rows, in_stride, ptr(si), ptr(win), len(win), ptr(out), ost, ptr(be), device)
    return (out, be) if biterr else out


def decode_tch_nblk_device(kind, n, d_type5, n_rows, in_stride, d_scramb, d_init_index, d_windows, n_blocks, d_n_blocks, d_type2, out_stride,
                           d_biterr=None, stream=None):
    """tetra_lmac_decode_tch_nblk_device: torch tensors on the GPU; d_init_index, d_n_blocks and d_biterr may be None."""
    call(_lib().tetra_lmac_decode_tch_nblk_device, int(kind), int(n), ptr(d_type5), int(n_rows), int(in_stride), ptr(d_scramb), ptr(d_init_index),
         ptr(d_windows), int(n_blocks), ptr(d_n_blocks), ptr(d_type2), int(out_stride), ptr(d_biterr), stream_ptr(stream))


def decode_tch_nblk_soft_device(kind, n, d_soft, n_rows, in_stride, d_scramb, d_init_index, d_windows, n_blocks, d_n_blocks, d_type2, out_stride,
                                d_biterr=None, stream=None):
    """tetra_lmac_decode_tch_nblk_soft_device: decode_tch_nblk_device on int8 soft values."""
    call(_lib().tetra_lmac_decode_tch_nblk_soft_device, int(kind), int(n), ptr(d_soft), int(n_rows), int(in_stride), ptr(d_scramb), ptr(d_init_index),
         ptr(d_windows), int(n_blocks), ptr(d_n_blocks), ptr(d_type2), int(out_stride), ptr(d_biterr), stream_ptr(stream))


def decode_batch_list(blk_type, type5, scramb=None, max_candidates=LIST_DEFAULT_CANDIDATES, device=-1):
    """tetra_lmac_decode_batch_list (include/ext/tetra_list.h): decode_batch plus the CRC-aided rescue of the failed rows
    -> (type2, crc_ok, rank int32 [n]: 0 = the decoder's own path passed, k >= 1 = rescued by candidate k, -1 = not rescued)."""
    rows, n, in_stride, si, out, ost, ok = _host_batch(blk_type, type5, scramb)
    rank = np.zeros(n, np.int32)
    call(_lib().tetra_lmac_decode_batch_list, int(blk_type), ptr(rows), n, in_stride, ptr(si), ptr(out), ost, ptr(ok), int(max_candidates), ptr(rank), device)
    return out, ok, rank


def decode_counted_list_device(blk_type, d_type5, capacity, d_n_blocks, in_stride, d_scramb, d_init_index, d_type2, out_stride, d_crc_ok,
                               max_candidates, d_rank, stream=None):
    """tetra_lmac_decode_counted_list_device: decode_counted_device plus max_candidates and d_rank (int32 tensor [capacity], or None)."""
    call(_lib().tetra_lmac_decode_counted_list_device, int(blk_type), ptr(d_type5), int(capacity), ptr(d_n_blocks), int(in_stride), ptr(d_scramb),
         ptr(d_init_index), ptr(d_type2), int(out_stride), ptr(d_crc_ok), int(max_candidates), ptr(d_rank), stream_ptr(stream))


def track_scramb_device(d_sb1_type2, type2_stride, d_crc_ok, d_valid, n_channels, frames_per_channel, d_chan_scramb, d_row_scramb,
                        stream=None):
    call(_lib().tetra_lmac_track_scramb_device, ptr(d_sb1_type2), int(type2_stride), ptr(d_crc_ok), ptr(d_valid), int(n_channels),
         int(frames_per_channel), ptr(d_chan_scramb), ptr(d_row_scramb), stream_ptr(stream))


def track_sync_device(d_sb1_type2, type2_stride, d_crc_ok, d_valid, d_n_frames, n_channels, frames_per_channel, d_cell, d_row_scramb,
                      d_row_time_rx=None, d_row_time=None, stream=None):
    """tetra_lmac_track_sync_device: d_cell = torch int32 / uint32 tensor [n_channels][10] (tetra_lmac_cell_state_t: scramb_init,
    colour_code, mcc, mnc, tcd tn / fn / mn, phy tn / fn / mn)."""
    call(_lib().tetra_lmac_track_sync_device, ptr(d_sb1_type2), int(type2_stride), ptr(d_crc_ok), ptr(d_valid), ptr(d_n_frames),
         int(n_channels), int(frames_per_channel), ptr(d_cell), ptr(d_row_scramb), ptr(d_row_time_rx), ptr(d_row_time), stream_ptr(stream))


def _job_array(jobs):
    arr = (Job * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        arr[i] = Job(int(j["type"]), int(j.get("blk_num", 0)), ptr(j.get("row_frame")), ptr(j.get("n_rows")), int(j["max_rows"]),
                     int(j.get("out_stride", 0)), ptr(j.get("frame_scramb")), ptr(j.get("type2")), ptr(j.get("crc_ok")), ptr(j.get("labels")))
    return arr


def decode_frames_workspace_bytes(jobs):
    """tetra_lmac_decode_frames_workspace_bytes (jobs as for decode_frames_device; only type and max_rows matter)."""
    return int(_lib().tetra_lmac_decode_frames_workspace_bytes(_job_array(jobs), len(jobs)))


def _frames(d_frames, d_frame_type, frames_per_channel, d_frame_bitnum, d_time_rx, d_time, d_workspace):
    """tetra_lmac_frames_t of torch tensors on the GPU (None: NULL)."""
    return Frames(ptr(d_frames), ptr(d_frame_type), int(d_frame_type.numel()), int(frames_per_channel), ptr(d_frame_bitnum), ptr(d_time_rx),
                  ptr(d_time), ptr(d_workspace), 0 if d_workspace is None else int(d_workspace.numel() * d_workspace.element_size()))


def decode_frames_device(d_frames, d_frame_type, jobs, frames_per_channel=0, d_frame_bitnum=None, d_time_rx=None, d_time=None, stream=None,
                         d_workspace=None):
    """tetra_lmac_decode_frames_device.  jobs: dicts with type, blk_num, row_frame, n_rows (tensor or None), max_rows, out_stride,
    frame_scramb (tensor or None), type2, crc_ok, labels (int32 tensor [rows][6] or None); d_workspace: uint8 tensor or None (pool)."""
    src = _frames(d_frames, d_frame_type, frames_per_channel, d_frame_bitnum, d_time_rx, d_time, d_workspace)
    call(_lib().tetra_lmac_decode_frames_device, C.byref(src), _job_array(jobs), len(jobs), stream_ptr(stream))


def decode_frames_biterr_device(d_frames, d_frame_type, jobs, frames_per_channel=0, d_frame_bitnum=None, d_time_rx=None, d_time=None, stream=None,
                                d_workspace=None, counted=True):
    """tetra_lmac_decode_frames_biterr_device: decode_frames_device whose jobs may carry `biterr` (int32 / uint32 tensor [max_rows], or
    None / absent: the job does not count).  counted=False hands in no array at all."""
    src = _frames(d_frames, d_frame_type, frames_per_channel, d_frame_bitnum, d_time_rx, d_time, d_workspace)
    arr = (vp * max(1, len(jobs)))(*[ptr(j.get("biterr")) for j in jobs])
    call(_lib().tetra_lmac_decode_frames_biterr_device, C.byref(src), _job_array(jobs), len(jobs), arr if counted else None, stream_ptr(stream))


def decode_frames_list_device(d_frames, d_frame_type, jobs, max_candidates=LIST_DEFAULT_CANDIDATES, frames_per_channel=0, d_frame_bitnum=None,
                              d_time_rx=None, d_time=None, stream=None, d_workspace=None, ranked=True):
    """tetra_lmac_decode_frames_list_device: decode_frames_device whose jobs may carry `rank` (int32 tensor [max_rows], or None / absent:
    the job is not rescued).  ranked=False hands in no array at all."""
    src = _frames(d_frames, d_frame_type, frames_per_channel, d_frame_bitnum, d_time_rx, d_time, d_workspace)
    arr = (vp * max(1, len(jobs)))(*[ptr(j.get("rank")) for j in jobs])
    call(_lib().tetra_lmac_decode_frames_list_device, C.byref(src), _job_array(jobs), len(jobs), int(max_candidates), arr if ranked else None,
         stream_ptr(stream))


def decode_frames_soft(d_frames, d_frame_type, jobs, d_ring, ring_size, frames_per_channel, d_frame_bitnum, max_candidates=LIST_DEFAULT_CANDIDATES,
                       d_time_rx=None, d_time=None, stream=None, d_workspace=None, counted=True, ranked=True):
    """tetra_lmac_decode_frames_soft_device (include/ext/tetra_soft.h): decode_frames_device whose coded kinds read soft values from
    d_ring (int8 tensor [channels][ring_size], or a raw device address) at the frames' bit numbers.  Jobs may carry `biterr` and `rank` as for
    decode_frames_biterr_device / decode_frames_list_device; counted=False / ranked=False hand in no array at all."""
    src = _frames(d_frames, d_frame_type, frames_per_channel, d_frame_bitnum, d_time_rx, d_time, d_workspace)
    counts = (vp * max(1, len(jobs)))(*[ptr(j.get("biterr")) for j in jobs])
    ranks = (vp * max(1, len(jobs)))(*[ptr(j.get("rank")) for j in jobs])
    call(_lib().tetra_lmac_decode_frames_soft_device, C.byref(src), _job_array(jobs), len(jobs), ptr(d_ring), int(ring_size),
         counts if counted else None, ranks if ranked else None, int(max_candidates), stream_ptr(stream))


def decode_frames_soft_tch(d_frames, d_frame_type, jobs, d_ring, ring_size, frames_per_channel, d_frame_bitnum, max_candidates=LIST_DEFAULT_CANDIDATES,
                           d_time_rx=None, d_time=None, stream=None, d_workspace=None, counted=True, ranked=True):
    """tetra_lmac_decode_frames_soft_tch_device (include/ext/tetra_tch_soft.h): decode_frames_soft whose jobs may also be of type T_TCH_4_8 /
    T_TCH_2_4 (no `rank` on those)."""
    src = _frames(d_frames, d_frame_type, frames_per_channel, d_frame_bitnum, d_time_rx, d_time, d_workspace)
    counts = (vp * max(1, len(jobs)))(*[ptr(j.get("biterr")) for j in jobs])
    ranks = (vp * max(1, len(jobs)))(*[ptr(j.get("rank")) for j in jobs])
    call(_lib().tetra_lmac_decode_frames_soft_tch_device, C.byref(src), _job_array(jobs), len(jobs), ptr(d_ring), int(ring_size),
         counts if counted else None, ranks if ranked else None, int(max_candidates), stream_ptr(stream))


def track_sync_lists_device(d_sb1_type2, type2_stride, d_crc_ok, d_frame_type, d_n_frames, d_chan_first_sync, n_channels, frames_per_channel,
                            d_cell, d_row_scramb, d_row_time_rx=None, d_row_time=None, d_frame_bitnum=None, d_sb1_labels=None, stream=None):
    """tetra_lmac_track_sync_lists_device (compact SB1 rows = the SYNC list's)."""
    call(_lib().tetra_lmac_track_sync_lists_device, ptr(d_sb1_type2), int(type2_stride), ptr(d_crc_ok), ptr(d_frame_type), ptr(d_n_frames),
         ptr(d_chan_first_sync), int(n_channels), int(frames_per_channel), ptr(d_cell), ptr(d_row_scramb), ptr(d_row_time_rx),
         ptr(d_row_time), ptr(d_frame_bitnum), ptr(d_sb1_labels), stream_ptr(stream))


def rm3014_decode_device(d_words, n, d_out_words, d_dist, stream=None):
    """tetra_lmac_rm3014_decode_device (include/tetra_aach.h): torch tensors on the GPU -- int32 / uint32 [n] 30-bit words in and out,
    uint8 [n] distances (0..3, or AACH_UNDECODABLE and the word unchanged)."""
    call(_lib().tetra_lmac_rm3014_decode_device, ptr(d_words), int(n), ptr(d_out_words), ptr(d_dist), stream_ptr(stream))


def decode_aach_rm3014_device(d_type5, n_blocks, in_stride, d_scramb, d_type2, out_stride, d_crc_ok, stream=None):
    """tetra_lmac_decode_aach_rm3014_device: decode_batch_device for TPSAP_T_BBK rows with the RM(30,14) decoding behind the
    descrambler; rows of >= 32 bytes out (30 bits, the distance, a zero)."""
    call(_lib().tetra_lmac_decode_aach_rm3014_device, ptr(d_type5), int(n_blocks), int(in_stride), ptr(d_scramb), ptr(d_type2),
         int(out_stride), ptr(d_crc_ok), stream_ptr(stream))


def job_aach_min_margin(m):
    """TETRA_LMAC_JOB_AACH_MIN_MARGIN(m): OR into the type of a TPSAP_T_BBK | JOB_RM3014_SOFT job; min_margin 1..930, 0 = absent = 1."""
    return (int(m) & 0x3ff) << 16


def rm3014_soft_decode(d_soft, n, soft_stride, d_out_words=None, d_dist=None, d_margin=None, stream=None):
    """tetra_lmac_rm3014_soft_decode_device (include/ext/tetra_aach_soft.h): torch tensors on the GPU -- int8 [n][soft_stride] soft values
    (30 of a row used, soft_stride >= 32) in; the maximum-likelihood codeword (int32 / uint32 [n]), the number of disagreeing non-zero
    values (uint8 [n]) and the margin to the runner-up (int16 / uint16 [n]) out, any of them None."""
    call(_lib().tetra_lmac_rm3014_soft_decode_device, ptr(d_soft), int(n), int(soft_stride), ptr(d_out_words), ptr(d_dist), ptr(d_margin),
         stream_ptr(stream))
