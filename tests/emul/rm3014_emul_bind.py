"""Builds and binds tests/emul/rm3014_emul.cpp (host build of the AACH's Reed-Muller lane code in lmac_core.hpp)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "librm3014_emul.so")
DEPS = [os.path.join(HERE, "rm3014_emul.cpp"), os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "lmac_core.hpp"),
        os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "demux_core.hpp")]

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "rm3014_emul.cpp"], DEPS, force=force)


def _load():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "rm3014_emul_encode": (None, [vp, i32, vp]),
            "rm3014_emul_syndrome": (None, [vp, i32, vp]),
            "rm3014_emul_decode": (None, [vp, i32, vp, vp]),
            "rm3014_emul_table": (i32, [vp]),
        })
    return _lib


def encode(info):
    """14 information bits (first bit on air at bit 13) -> the 30-bit codeword, information in bits 29..16, parity in 15..0."""
    v = np.ascontiguousarray(info, np.uint32).reshape(-1)
    out = np.zeros(v.size, np.uint32)
    _load().rm3014_emul_encode(v.ctypes.data_as(C.c_void_p), int(v.size), out.ctypes.data_as(C.c_void_p))
    return out


def syndrome(words):
    v = np.ascontiguousarray(words, np.uint32).reshape(-1)
    out = np.zeros(v.size, np.uint32)
    _load().rm3014_emul_syndrome(v.ctypes.data_as(C.c_void_p), int(v.size), out.ctypes.data_as(C.c_void_p))
    return out


def decode(words):
    """rm3014_decode per word -> (words', dist uint8): the codeword within distance 3 and the distance, else the word and 0xFF."""
    v = np.ascontiguousarray(words, np.uint32).reshape(-1)
    out, dist = np.zeros(v.size, np.uint32), np.zeros(v.size, np.uint8)
    _load().rm3014_emul_decode(v.ctypes.data_as(C.c_void_p), int(v.size), out.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p))
    return out, dist


def table():
    """-> (the correction table uint32 [65536], the number of syndromes that have an error pattern)."""
    out = np.zeros(1 << 16, np.uint32)
    have = _load().rm3014_emul_table(out.ctypes.data_as(C.c_void_p))
    return out, int(have)
