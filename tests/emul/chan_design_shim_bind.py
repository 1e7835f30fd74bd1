"""ctypes binding of tests/emul/chan_design_shim.cpp (the product's window design, csrc/chan_design.hpp, built for the host; TEST TOOL)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
_SO = os.path.join(_HERE, "libchan_design_shim.so")
_lib = None


def build():
    return hostlib.build(_SO, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "chan_design_shim.cpp", "-o", hostlib.OUT],
                         [os.path.join(_HERE, "chan_design_shim.cpp"), os.path.join(_CSRC, "chan_design.hpp")])


def kaiser_sinc(L, fc, beta, gain):
    """chandesign::kaiser_sinc -> float32 [L]."""
    global _lib
    if _lib is None:
        _lib = hostlib.load(build(), {"chan_design_shim": (None, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p])})
    out = np.zeros(L, np.float32)
    _lib.chan_design_shim(L, fc, beta, gain, out.ctypes.data)
    return out
