"""ctypes binding of the batched training-sequence search (include/tetra_burst_scan.h)."""
import ctypes as C
import functools

import numpy as np

from ._ffi import P, call, declare, i32, ptr, stream_ptr, u32, vp
from .binding import load_library

# include/tetra_burst_scan.h
SIGNATURES = {
    "tetra_find_train_seq_batch_device": (i32, [vp, i32, i32, vp, u32, vp, vp, vp]),
    "tetra_find_train_seq_batch": (i32, [vp, i32, i32, vp, u32, vp, vp, i32]),
    "tetra_ts_indicator_create": (i32, [i32, i32, P(vp)]),
    "tetra_ts_indicator_destroy": (None, [vp]),
    "tetra_ts_indicator_reset": (i32, [vp, i32]),
    "tetra_ts_indicator_process_device": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "tetra_ts_indicator_process": (i32, [vp, vp, i32, vp, vp, vp]),
}
SCAN_EXPORTS = [n for n in SIGNATURES if n != "tetra_ts_indicator_destroy"]      # (the entry points that return a status)
TRAIN_NORM_1, TRAIN_NORM_2, TRAIN_NORM_3, TRAIN_SYNC, TRAIN_EXT = 0, 1, 2, 3, 4
ALL_MASK = 0x1f


@functools.lru_cache(None)
def _lib():
    return declare(load_library(), SIGNATURES)


def find_train_seq_batch(bits, end_of_in, mask=ALL_MASK, device=-1):
    """bits uint8 [C][stride] (stride % 4 == 0), end_of_in int32 [C] -> (type int32 [C], offset int32 [C])."""
    bits = np.ascontiguousarray(bits, np.uint8)
    end = np.ascontiguousarray(end_of_in, np.int32)
    Cn, stride = bits.shape
    t = np.zeros(Cn, np.int32)
    o = np.zeros(Cn, np.int32)
    call(_lib().tetra_find_train_seq_batch, ptr(bits), Cn, stride, ptr(end), int(mask), ptr(t), ptr(o), device)
    return t, o


def find_train_seq_batch_device(d_bits, n_channels, bits_stride, d_end, mask, d_type, d_offset, stream=None):
    call(_lib().tetra_find_train_seq_batch_device, ptr(d_bits), int(n_channels), int(bits_stride), ptr(d_end), int(mask), ptr(d_type),
         ptr(d_offset), stream_ptr(stream))


class TsIndicator:
    """The plugin's training-sequence indicator (src/main.cpp:385-414) for C channels on one GPU, state carried."""

    def __init__(self, n_channels, device=-1):
        self._h = C.c_void_p()
        call(_lib().tetra_ts_indicator_create, int(n_channels), int(device), C.byref(self._h))
        self.n_channels = int(n_channels)

    def close(self):
        if self._h:
            _lib().tetra_ts_indicator_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, channel=-1):
        call(_lib().tetra_ts_indicator_reset, self._h, int(channel))

    def process(self, bits, n_bits):
        """bits uint8 [C][stride] (stride % 4 == 0), n_bits int32 [C] -> (found bool [C], expire int32 [C])."""
        b = np.ascontiguousarray(bits, np.uint8)
        nb = np.ascontiguousarray(n_bits, np.int32)
        assert b.shape[0] == self.n_channels and nb.shape[0] == self.n_channels
        found = np.zeros(self.n_channels, np.uint8)
        expire = np.zeros(self.n_channels, np.int32)
        call(_lib().tetra_ts_indicator_process, self._h, ptr(b), b.shape[1], ptr(nb), ptr(found), ptr(expire))
        return found.astype(bool), expire

    def process_device(self, d_bits, bits_stride, d_n_bits, d_found, d_expire=None, stream=None):
        call(_lib().tetra_ts_indicator_process_device, self._h, ptr(d_bits), int(bits_stride), ptr(d_n_bits), ptr(d_found), ptr(d_expire),
             stream_ptr(stream))
