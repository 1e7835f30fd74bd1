"""Builds and binds tests/emul/aach_soft_emul.cpp (host build of the soft AACH decoder's lane code, csrc/soft_core.hpp)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libaach_soft_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "aach_soft_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + [os.path.join(CSRC, f) for f in ("soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "aach_soft_emul.cpp"], DEPS, force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "aach_soft_emul_max_margin": (i32, []),
            "aach_soft_emul_stage": (i32, [vp, C.c_uint32, vp, vp, i32, vp, vp]),
            "aach_soft_emul_decode": (None, [vp, i32, i32, vp, vp, vp]),
            "aach_soft_emul_rows": (None, [vp, i32, i32, i32, vp, vp]),
        })
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def max_margin():
    return int(lib().aach_soft_emul_max_margin())


def stage(rings, bitnum, frame_type, scramb):
    """aach_soft_block per row: rings int8 [n][R] (R a power of two), the frames' bit numbers, burst types and scrambling codes
    -> int8 [n][32]: the 30 descrambled soft values and two zeros."""
    rg = np.ascontiguousarray(rings, np.int8)
    n, R = rg.shape
    bn, ft, sc = (np.ascontiguousarray(a, t) for a, t in ((bitnum, np.uint32), (frame_type, np.int32), (scramb, np.uint32)))
    assert len(bn) == len(ft) == len(sc) == n
    out = np.zeros((n, 32), np.int8)
    assert lib().aach_soft_emul_stage(_p(rg), R, _p(bn), _p(ft), n, _p(sc), _p(out)) == 0
    return out


def decode(soft):
    """soft int8 [n][>= 32] -> (codewords uint32 [n], dist uint8 [n], margin uint16 [n])."""
    rows = np.ascontiguousarray(soft, np.int8)
    n, stride = rows.shape
    words, dist, margin = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    lib().aach_soft_emul_decode(_p(rows), n, stride, _p(words), _p(dist), _p(margin))
    return words, dist, margin


def rows(soft, min_margin=1):
    """soft int8 [n][>= 32] -> (rows uint8 [n][32], crc_ok int32 [n]) as the frame decoder's soft BBK job writes them."""
    sv = np.ascontiguousarray(soft, np.int8)
    n, stride = sv.shape
    out, ok = np.zeros((n, 32), np.uint8), np.zeros(n, np.int32)
    lib().aach_soft_emul_rows(_p(sv), n, stride, int(min_margin), _p(out), _p(ok))
    return out, ok
