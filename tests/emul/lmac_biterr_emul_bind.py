"""Builds and binds tests/emul/lmac_biterr_emul.cpp (host build of the channel bit-error count's lane code, csrc/lmac_core.hpp
reencode_errors, behind the decoder's three front ends)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib
from tests.soft_pipeline import KINDS, TYPE2_BITS, lay_rings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_biterr_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "lmac_biterr_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + [os.path.join(CSRC, f) for f in ("soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_biterr_emul.cpp"], DEPS,
                         force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "biterr_emul_rows": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, vp, i32, C.POINTER(C.c_int32)]),
            "biterr_emul_frames": (i32, [i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]),
            "biterr_emul_soft": (i32, [i32, i32, vp, C.c_uint32, vp, vp, i32, vp, vp, i32, vp, vp]),
        })
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def split(biterr):
    """errors | compared << 16 -> (errors, compared)"""
    v = np.asarray(biterr, np.uint32)
    return (v & 0xffff).astype(np.int64), (v >> 16).astype(np.int64)


def decode_rows(blk_type, type5, scramb, route=0):
    """k_lmac_decode's lane code with counts, a 64-row workgroup at a time (route 1: the byte route forced)
    -> (rows [n][type2], crc_ok, biterr uint32 [n], the rows of the workgroups that took the packed route)."""
    rows = np.ascontiguousarray(type5, np.uint8)
    n, stride = rows.shape
    si = None if scramb is None else np.ascontiguousarray(scramb, np.uint32)
    n2 = {0: 80, 1: 144, 2: 144, 4: 112, 5: 288}[int(blk_type)]
    out, ok, be = np.zeros((n, n2), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    fast = C.c_int32(-1)
    rc = lib().biterr_emul_rows(int(blk_type), _p(rows), n, stride, _p(si), _p(out), n2, _p(ok), _p(be), int(route), C.byref(fast))
    assert rc == 0
    return out, ok, be, fast.value


def decode_frames(tpsap, blk_num, frames_packed, frame_type, row_frame, frame_scramb, out_stride):
    """The lane code of k_lmac_frames with counts, one job of a coded kind -> (rows [n][out_stride], crc_ok, biterr)."""
    fr = np.ascontiguousarray(frames_packed, np.uint32)
    ft = np.ascontiguousarray(frame_type, np.int32)
    rf = np.ascontiguousarray(row_frame, np.int32)
    sc = None if frame_scramb is None else np.ascontiguousarray(frame_scramb, np.uint32)
    out, ok, be = np.zeros((rf.size, out_stride), np.uint8), np.zeros(rf.size, np.int32), np.zeros(rf.size, np.uint32)
    rc = lib().biterr_emul_frames(int(tpsap), int(blk_num), _p(fr), _p(ft), _p(rf), rf.size, _p(sc), _p(out), out_stride, _p(ok), _p(be))
    if rc:
        raise ValueError("refused")
    return out, ok, be


def decode_soft_rows(kind, soft_rows, scramb=None, ring=1024, bitnum=None):
    """One lane of k_lmac_frames_soft with counts per row; rows laid into rings as lmac_soft_emul_bind.decode_rows does
    -> (type-2 bits uint8 [n][type2], crc_ok int32 [n], biterr uint32 [n])."""
    tpsap, blk, train, pieces = KINDS[kind]
    rows = np.ascontiguousarray(soft_rows, np.int8)
    n = len(rows)
    rings, bn = lay_rings(kind, rows, ring, bitnum)
    ft = np.full(n, train, np.int32)
    sc = None if scramb is None else np.ascontiguousarray(scramb, np.uint32)
    n2 = TYPE2_BITS[kind]
    out, ok, be = np.zeros((n, n2), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    rc = lib().biterr_emul_soft(tpsap, blk, _p(rings), ring, _p(bn), _p(ft), n, _p(sc), _p(out), n2, _p(ok), _p(be))
    assert rc == 0
    return out, ok, be
