"""ctypes binding of tests/emul/resamp_emul.cpp (host emulation of the rational resampler's kernels, over every column and over
picked columns; TEST TOOL)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "libresamp_emul.so")
_lib = None


def build():
    return hostlib.build(_SO, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "resamp_emul.cpp", "-o", hostlib.OUT],
                         [os.path.join(_HERE, "resamp_emul.cpp")] + [os.path.join(_ROOT, "sdrpp-tetra-demodulator_amd", "csrc", f) for f in ("resamp_core.hpp",)])


def lib():
    global _lib
    if _lib is None:
        vp, i32, i64 = C.c_void_p, C.c_int, C.c_longlong
        _lib = hostlib.load(build(), {"resamp_emul": (i32, [i32] * 6 + [vp, vp, vp, i32, i64, i64, vp, i32, vp]),
                                      "resamp_emul_ratios": (i32, [vp, i32])})
    return _lib


def ratios():
    """The (I, DN, T) the product has specialised kernels for, read from its own table (resamp_core.hpp)."""
    out = np.zeros((lib().resamp_emul_ratios(None, 0), 3), np.int32)
    lib().resamp_emul_ratios(out.ctypes.data, len(out))
    return [tuple(int(v) for v in r) for r in out]


class ResampEmul:
    """The resampler kernels' arithmetic and index maps with the C ABI's carried state (delay line of T - 1 frames, positions).
    cols: None, or the picked columns of input rows of n_channels channels (output column j = input column cols[j]; the delay line
    holds the picked columns)."""

    def __init__(self, n_channels, I, DN, T, proto, generic=False, W=None, cols=None):
        self.in_ch, self.I, self.DN, self.T = n_channels, I, DN, T
        self.cols = None if cols is None else np.ascontiguousarray(cols, np.int32)
        self.C = n_channels if cols is None else self.cols.size
        self.W = 2 if cols is not None else W if W is not None else (4 if n_channels % 2 == 0 else 2)
        self.h = np.ascontiguousarray(proto, np.float32)
        self.generic = generic
        self.hist = np.zeros((T - 1, self.C), np.complex64)
        self.n_total, self.m_next = 0, 0

    def process(self, x):
        x = np.ascontiguousarray(x, np.complex64).reshape(-1, self.in_ch)
        n_in = x.shape[0]
        m1 = ((self.n_total + n_in) * self.I + self.DN - 1) // self.DN
        n_out = m1 - self.m_next
        # exact-size buffers in their own allocations, NaN-poisoned output: every stored element must be written, nothing beyond
        out = np.full((max(n_out, 1), self.C), np.nan + 0j, np.complex64)
        xs = x.copy() if n_in else np.zeros((1, self.in_ch), np.complex64)
        got = lib().resamp_emul(self.I, self.DN, self.T, self.C, self.W, int(self.generic), self.h.ctypes.data, self.hist.ctypes.data,
                                xs.ctypes.data, n_in, self.n_total, self.m_next, out.ctypes.data, self.in_ch,
                                None if self.cols is None else self.cols.ctypes.data)
        assert got == n_out, (got, n_out)
        self.hist = np.concatenate([self.hist, x if self.cols is None else x[:, self.cols]])[n_in:].copy()
        self.n_total += n_in
        self.m_next = m1
        return out[:n_out]


class ResampSelectEmul(ResampEmul):
    """The selecting resampler of the wideband receiver: input rows of in_ch channels, output column j = input column cols[j]."""

    def __init__(self, in_ch, cols, I, DN, T, proto, generic=False):
        super().__init__(in_ch, I, DN, T, proto, generic=generic, cols=cols)
