"""Builds and binds tests/emul/lmac_tch_emul.cpp (host build of the circuit-mode data channels' lane code, csrc/tch_core.hpp, behind
the decoder's front ends)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_tch_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "lmac_tch_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + [os.path.join(CSRC, f) for f in ("tch_core.hpp", "lmac_core.hpp", "demux_core.hpp")]
TCH_7_2, TCH_4_8, TCH_2_4 = 8, 9, 10
TYPE2 = {TCH_7_2: 432, TCH_4_8: 292, TCH_2_4: 148}

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_tch_emul.cpp"], DEPS,
                         force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "tch_emul_rows": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, i32, C.POINTER(C.c_int32)]),
            "tch_emul_frames": (i32, [i32, vp, vp, vp, i32, vp, vp, i32, vp]),
            "tch_emul_schedule": (i32, [i32, vp]),
        })
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def decode_rows(kind, type5, scramb, route=0, biterr=True):
    """k_tch_rows' lane code, a 64-row workgroup at a time (route 1: the byte route forced)
    -> (rows [n][type2], biterr uint32 [n] or None, the rows of the workgroups that took the packed route)."""
    rows = np.ascontiguousarray(type5, np.uint8)
    n, stride = rows.shape
    si = np.ascontiguousarray(scramb, np.uint32)
    n2 = TYPE2[int(kind)]
    out = np.zeros((n, n2), np.uint8)
    be = np.zeros(n, np.uint32) if biterr else None
    fast = C.c_int32(-1)
    rc = lib().tch_emul_rows(int(kind), _p(rows), n, stride, _p(si), _p(out), n2, _p(be), int(route), C.byref(fast))
    assert rc == 0
    return out, be, fast.value


def decode_frames(kind, frames_packed, frame_type, row_frame, frame_scramb, out_stride, biterr=True):
    """k_tch_frames' lane code, one job -> (rows [n][out_stride], biterr or None)."""
    fr = np.ascontiguousarray(frames_packed, np.uint32)
    ft = np.ascontiguousarray(frame_type, np.int32)
    rf = np.ascontiguousarray(row_frame, np.int32)
    sc = np.ascontiguousarray(frame_scramb, np.uint32)
    out = np.zeros((rf.size, out_stride), np.uint8)
    be = np.zeros(rf.size, np.uint32) if biterr else None
    rc = lib().tch_emul_frames(int(kind), _p(fr), _p(ft), _p(rf), rf.size, _p(sc), _p(out), out_stride, _p(be))
    assert rc == 0
    return out, be


def schedule(kind):
    """pair_pattern of every step pair: uint8 [type2 / 2], g1 g2 g3 g4 of the even step in bits 7..4, of the odd step in bits 3..0."""
    pat = np.zeros(TYPE2[int(kind)] // 2, np.uint8)
    n = lib().tch_emul_schedule(int(kind), _p(pat))
    assert n == pat.size
    return pat
