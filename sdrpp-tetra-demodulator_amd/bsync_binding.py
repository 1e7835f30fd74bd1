"""ctypes binding of the batched burst synchroniser + burst demultiplexer (include/tetra_burst_sync.h)."""
import ctypes as C
import functools

import numpy as np

from ._ffi import P, call, declare, i32, ptr, stream_ptr, vp
from .binding import load_library

LIST_SYNC, LIST_NORM_1, LIST_NORM_2, LIST_ANY, N_LISTS = 0, 1, 2, 3, 4
FRAME_WORDS = 16
RX_S_UNLOCKED, RX_S_KNOW_FSTART, RX_S_LOCKED = 0, 1, 2
FRAME_STRIDE, FRAME_NONE, BITS_PER_TS = 512, -2, 510


class BsyncState(C.Structure):
    _fields_ = [("state", C.c_int32), ("bits_in_buf", C.c_uint32), ("bitbuf_start_bitnum", C.c_uint32),
                ("next_frame_start_bitnum", C.c_uint32)]


# include/tetra_burst_sync.h
SIGNATURES = {
    "tetra_bsync_create": (i32, [i32, i32, i32, P(vp)]),
    "tetra_bsync_destroy": (i32, [vp]),
    "tetra_bsync_reset": (i32, [vp]),
    "tetra_bsync_max_frames": (i32, [vp]),
    "tetra_bsync_process_device": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    "tetra_bsync_process_packed_device": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, vp]),
    "tetra_bsync_process": (i32, [vp, vp, i32, vp, vp, vp, vp, vp]),
    "tetra_bsync_get_state": (i32, [vp, i32, i32, P(BsyncState)]),
    "tetra_burst_demux_device": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp]),
    "tetra_burst_demux_compact_device": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "tetra_burst_demux_packed_device": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp]),
    "tetra_burst_demux_compact_packed_device": (i32, [vp, vp, i32, i32, i32, vp, i32, vp, vp, vp]),
    "tetra_burst_index_device": (i32, [vp, i32, i32, vp, vp, vp, vp, vp]),
}
BSYNC_EXPORTS = list(SIGNATURES)


class BsyncTolerance(C.Structure):
    """tetra_bsync_tolerance_t."""
    _fields_ = [("tol_norm", C.c_int32), ("tol_sync", C.c_int32), ("max_miss", C.c_int32)]


# include/ext/tetra_sync_tol.h (the tolerant lock): the synchroniser's share
SYNC_TOL_ABI = {
    "tetra_bsync_set_tolerance": (i32, [vp, P(BsyncTolerance)]),
    "tetra_bsync_get_misses": (i32, [vp, i32, i32, vp]),
}
SYNC_TOL_DEFAULT = (3, 5, 16)


def tolerance_arg(tol):
    """None -> NULL (the reference's rule); (tol_norm, tol_sync, max_miss) -> a tetra_bsync_tolerance_t."""
    return None if tol is None else C.byref(BsyncTolerance(*[int(v) for v in tol]))


@functools.lru_cache(None)
def _lib():
    # (a TETRA_DEMOD_LIB override may be an older build without the tolerant lock)
    return declare(load_library(), {**SIGNATURES, **SYNC_TOL_ABI}, optional=list(SYNC_TOL_ABI))


class BurstSync:
    """C independent tetra_rx_state receivers on one GPU."""

    def __init__(self, n_channels, max_bits, device=-1):
        self._h = C.c_void_p()
        call(_lib().tetra_bsync_create, int(n_channels), int(max_bits), int(device), C.byref(self._h))
        self.n_channels, self.max_bits = int(n_channels), int(max_bits)
        self.max_frames = _lib().tetra_bsync_max_frames(self._h)

    def close(self):
        if self._h:
            _lib().tetra_bsync_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        call(_lib().tetra_bsync_reset, self._h)

    def process(self, bits, n_bits):
        """bits uint8 [C][stride] (stride % 4 == 0), n_bits int32 [C] -> (frames uint8 [C][F][512], frame_type int32 [C][F],
        frame_bitnum uint32 [C][F], n_frames int32 [C])."""
        b = np.ascontiguousarray(bits, np.uint8)
        nb = np.ascontiguousarray(n_bits, np.int32)
        Cn, F = self.n_channels, self.max_frames
        assert b.shape[0] == Cn and nb.shape[0] == Cn
        frames = np.zeros((Cn, F, FRAME_STRIDE), np.uint8)
        ft = np.zeros((Cn, F), np.int32)
        fb = np.zeros((Cn, F), np.uint32)
        nf = np.zeros(Cn, np.int32)
        call(_lib().tetra_bsync_process, self._h, ptr(b), b.shape[1], ptr(nb), ptr(frames), ptr(ft), ptr(fb), ptr(nf))
        return frames, ft, fb, nf

    def process_device(self, d_bits, bits_stride, d_n_bits, d_frames, d_frame_type, d_frame_bitnum, d_n_frames, stream=None):
        call(_lib().tetra_bsync_process_device, self._h, ptr(d_bits), int(bits_stride), ptr(d_n_bits), ptr(d_frames), ptr(d_frame_type),
             ptr(d_frame_bitnum), ptr(d_n_frames), stream_ptr(stream))

    def process_packed_device(self, d_bits, bits_stride, d_n_bits, d_frames_packed, d_frame_type, d_frame_bitnum, d_n_frames, stream=None):
        """Frames as [C][max_frames][16] int32 / uint32 words (first bit = most significant) instead of [C][max_frames][512] bytes."""
        call(_lib().tetra_bsync_process_packed_device, self._h, ptr(d_bits), int(bits_stride), ptr(d_n_bits), ptr(d_frames_packed),
             ptr(d_frame_type), ptr(d_frame_bitnum), ptr(d_n_frames), stream_ptr(stream))

    def set_tolerance(self, tol):
        """tetra_bsync_set_tolerance: (tol_norm, tol_sync, max_miss) from the next process call on, None = the reference's rule."""
        call(_lib().tetra_bsync_set_tolerance, self._h, tolerance_arg(tol))

    def misses(self, first=0, count=None):
        """tetra_bsync_get_misses: int32 [count], the channels' consecutive LOCKED frames without a training sequence."""
        count = self.n_channels - first if count is None else count
        out = np.zeros(max(count, 1), np.int32)
        call(_lib().tetra_bsync_get_misses, self._h, int(first), int(count), ptr(out))
        return out[:count]

    def states(self, first=0, count=None):
        count = self.n_channels - first if count is None else count
        arr = (BsyncState * count)()
        call(_lib().tetra_bsync_get_state, self._h, int(first), int(count), arr)
        return [(s.state, s.bits_in_buf, s.bitbuf_start_bitnum, s.next_frame_start_bitnum) for s in arr]


def demux_compact_device(d_frames, d_frame_type, n, tpsap, blk_num, d_rows, row_stride, d_row_frame, d_n_rows, stream=None, packed=False):
    fn = _lib().tetra_burst_demux_compact_packed_device if packed else _lib().tetra_burst_demux_compact_device
    call(fn, ptr(d_frames), ptr(d_frame_type), int(n), int(tpsap), int(blk_num), ptr(d_rows), int(row_stride), ptr(d_row_frame), ptr(d_n_rows),
         stream_ptr(stream))


def demux_device(d_frames, d_frame_type, n, tpsap, blk_num, d_rows, row_stride, d_valid, stream=None, packed=False):
    fn = _lib().tetra_burst_demux_packed_device if packed else _lib().tetra_burst_demux_device
    call(fn, ptr(d_frames), ptr(d_frame_type), int(n), int(tpsap), int(blk_num), ptr(d_rows), int(row_stride), ptr(d_valid), stream_ptr(stream))


def index_device(d_frame_type, frames_per_channel, d_lists, d_counts, d_chan_first=None, d_work=None, stream=None):
    """tetra_burst_index_device: d_lists [4][n], d_counts [4], d_chan_first [4][n / frames_per_channel] or None (int32 tensors)."""
    import torch
    n = int(d_frame_type.numel())
    if d_work is None:
        d_work = torch.empty(N_LISTS * ((n + 255) // 256) + 1, dtype=torch.int32, device=d_frame_type.device)
    call(_lib().tetra_burst_index_device, ptr(d_frame_type), n, int(frames_per_channel), ptr(d_lists), ptr(d_counts),  # (empty tensors: NULL)
         ptr(d_chan_first), ptr(d_work), stream_ptr(stream))
