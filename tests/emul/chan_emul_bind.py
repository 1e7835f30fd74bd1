"""ctypes binding of tests/emul/chan_emul.cpp (host emulation of the channeliser's FFT kernel, un-shifted and frequency-shifted;
TEST TOOL).  Compiles on first use."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libchan_emul.so")
_lib = None


def build():
    return hostlib.build(_SO, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "chan_emul.cpp", "-o", hostlib.OUT],
                         [os.path.join(_HERE, "chan_emul.cpp")] + [os.path.join(_ROOT, "sdrpp-tetra-demodulator_amd", "csrc", f) for f in ("chan_fft_core.hpp",)])


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "chan_fft_emul": (i32, [vp, vp, i32, i32, i32, i32, C.c_longlong, vp, C.c_uint, i32, vp]),
            "chan_shift_phasor": (None, [C.c_uint, vp]),
            "chan_shift_taps": (None, [vp, i32, C.c_uint, vp, vp]),
            "chan_fft32": (None, [vp, vp]),
            "chan_dft25": (None, [vp, vp]),
        })
    return _lib


def phasor(ph):
    out = np.zeros(2, np.float32)
    lib().chan_shift_phasor(int(ph) & 0xffffffff, out.ctypes.data)
    return complex(out[0], out[1])


def shift_taps(P, proto, inc):
    """The modulated taps as tetra_chan_set_shift lays them out: ([L], [800][2][P]) complex64."""
    h = np.ascontiguousarray(proto, np.float32)
    lin, fold = np.zeros(800 * P, np.complex64), np.zeros((800, 2, P), np.complex64)
    lib().chan_shift_taps(h.ctypes.data, P, int(inc) & 0xffffffff, lin.ctypes.data, fold.ctypes.data)
    return lin, fold


class ChanFftShiftEmul:
    """The FFT kernel's arithmetic for M = 800, D = 400, P taps per channel, with the handle's carried state: delay line, sub-frame
    phase, absolute position (the phase reference) and the shift.  force_shift_code: run the SHIFT = true lane code even for inc == 0
    (the library dispatches inc == 0 to the un-shifted kernels)."""

    def __init__(self, P, proto, inc=0, force_shift_code=False):
        self.P, self.L = P, 800 * P
        self.h = np.ascontiguousarray(proto, np.float32)
        self.hist = np.zeros(self.L - 1, np.complex64)
        self.phase, self.consumed = 0, 0
        self.inc, self.mode = int(inc) & 0xffffffff, int(bool(force_shift_code))

    def set_shift(self, inc):
        self.inc = int(inc) & 0xffffffff

    def process(self, x):
        """x: complex64 samples, or integer I / Q pairs [n][2] int16 / int8 (tetra_chan_process_device_cs16 / _cs8)."""
        x = np.ascontiguousarray(x)
        if x.dtype == np.int16 or x.dtype == np.int8:
            fmt = 1 if x.dtype == np.int16 else 2
            xc = (x[:, 0].astype(np.float32) + 1j * x[:, 1].astype(np.float32)).astype(np.complex64) / np.float32(32768 if fmt == 1 else 128)
        else:
            fmt, x = 0, np.ascontiguousarray(x, np.complex64)
            xc = x
        frames = (self.phase + len(x)) // 400
        out = np.full((max(frames, 1), 800), np.nan + 0j, np.complex64)      # every stored element must be written
        # exact-size buffers in their own allocations (no slack behind the new samples: the kernel must not read past them)
        xs = x.copy() if len(x) else np.zeros((1, 2), x.dtype) if fmt else np.zeros(1, np.complex64)
        got = lib().chan_fft_emul(self.hist.ctypes.data, xs.ctypes.data, fmt, len(x), self.P, self.phase, self.consumed, self.h.ctypes.data,
                                  self.inc, self.mode, out.ctypes.data)
        assert got == frames
        self.hist = np.concatenate([self.hist, xc])[len(xc):].copy()
        self.phase = (self.phase + len(x)) % 400
        self.consumed += len(x)
        return out[:frames]


class ChanFftEmul(ChanFftShiftEmul):
    """The un-shifted kernel: no shift, the library's dispatch."""

    def __init__(self, P, proto):
        super().__init__(P, proto)


def fft32(x):
    x = np.ascontiguousarray(x, np.complex64)
    y = np.zeros(32, np.complex64)
    lib().chan_fft32(x.ctypes.data, y.ctypes.data)
    return y


def dft25(x):
    x = np.ascontiguousarray(x, np.complex64)
    y = np.zeros(25, np.complex64)
    lib().chan_dft25(x.ctypes.data, y.ctypes.data)
    return y
