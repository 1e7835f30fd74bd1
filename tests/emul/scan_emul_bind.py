"""Builds and binds tests/emul/scan_emul.cpp (host build of the training-sequence search's and the indicator's lane code,
csrc/scan_core.hpp)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libscan_emul.so")
DEPS = [os.path.join(HERE, "scan_emul.cpp"), os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "scan_core.hpp")]

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "scan_emul.cpp"], DEPS, force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "scan_emul_find": (None, [vp, i32, i32, vp, C.c_uint32, vp, vp, vp]),
            "scan_emul_indicator": (None, [vp, i32, i32, vp, vp, vp, vp, vp]),
            "scan_emul_trace": (None, [vp, i32]),
            "scan_emul_tile": (i32, []),
            "scan_emul_ind_tile": (i32, []),
        })
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def tile():
    return int(lib().scan_emul_tile())


def ind_tile():
    return int(lib().scan_emul_ind_tile())


def rows_at(rows, offset=0):
    """A copy of rows uint8 [C][stride] whose first byte lies `offset` bytes past a 64-byte boundary, with 64 guard bytes of 1
    before it and after it (the same memory a device buffer with an offset base gives the kernel)."""
    r = np.ascontiguousarray(rows, np.uint8)
    buf = np.ones(r.size + 256, np.uint8)
    at = (-buf.ctypes.data) % 64 + 64 + int(offset)
    view = buf[at:at + r.size].reshape(r.shape)
    view[...] = r
    assert view.ctypes.data % 64 == offset % 64
    return view


def trace(reset=True):
    """Words packed by {16-byte, dword, byte} loads since the last reset, and loads the hardware could not have made as one access."""
    out = np.zeros(4, np.int64)
    lib().scan_emul_trace(_p(out), int(reset))
    return dict(route16=int(out[0]), route4=int(out[1]), route1=int(out[2]), misaligned=int(out[3]))


def find_train_seq_batch(bits, end_of_in, mask=0x1f):
    """k_find_train_seq on bits uint8 [C][stride] (used where it lies: its address decides the packing route) ->
    (type int32 [C], offset int32 [C], tiles packed int32 [C])."""
    assert bits.dtype == np.uint8 and bits.flags.c_contiguous and bits.shape[1] % 4 == 0 and bits.ctypes.data % 4 == 0
    end = np.ascontiguousarray(end_of_in, np.int32)
    Cn, stride = bits.shape
    assert end.size == Cn
    t, o, tiles = np.zeros(Cn, np.int32), np.zeros(Cn, np.int32), np.zeros(Cn, np.int32)
    lib().scan_emul_find(_p(bits), Cn, stride, _p(end), int(mask), _p(t), _p(o), _p(tiles))
    return t, o, tiles


class TsIndicator:
    """k_ts_indicator with the handle's carried state: same interface as scan_binding.TsIndicator."""

    def __init__(self, n_channels):
        self.n_channels = int(n_channels)
        self.reset()

    def reset(self, channel=-1):
        if channel < 0:
            self.tail = np.zeros((self.n_channels, 44), np.uint8)
            self.expire = np.zeros(self.n_channels, np.int32)
        else:
            self.tail[channel] = 0
            self.expire[channel] = 0

    def process(self, bits, n_bits, want_expire=True):
        assert bits.dtype == np.uint8 and bits.flags.c_contiguous and bits.shape[1] % 4 == 0 and bits.ctypes.data % 4 == 0
        nb = np.ascontiguousarray(n_bits, np.int32)
        assert bits.shape[0] == self.n_channels and nb.size == self.n_channels
        found = np.zeros(self.n_channels, np.uint8)
        expire = np.zeros(self.n_channels, np.int32)
        lib().scan_emul_indicator(_p(bits), self.n_channels, bits.shape[1], _p(nb), _p(self.tail), _p(self.expire), _p(found),
                                  _p(expire) if want_expire else None)
        return found.astype(bool), (expire if want_expire else None)
