"""Builds and binds tests/emul/lmac_list_emul.cpp (host build of the CRC-aided list decoding's lane code, csrc/list_core.hpp, behind the
decoder's three front ends)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib
from tests.soft_pipeline import KINDS, TYPE2_BITS, lay_rings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_list_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "lmac_list_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + \
    [os.path.join(CSRC, f) for f in ("list_core.hpp", "soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]
N2 = {0: 80, 1: 144, 2: 144, 4: 112, 5: 288}

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_list_emul.cpp"], DEPS,
                         force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "list_emul_rows": (i32, [i32, vp, i32, i32, vp, vp, i32, vp, vp, vp, i32, i32, i32]),
            "list_emul_frames": (i32, [i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32]),
            "list_emul_soft": (i32, [i32, i32, vp, C.c_uint32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32]),
        })
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def decode_rows(blk_type, type5, scramb, T, route=0, bits_rescue=False):
    """A decode launch with ranks on byte rows, a 64-row workgroup at a time (route 1: the byte route forced; bits_rescue: the rescue
    stages plain rows as packed bits) -> (rows [n][type2], crc_ok, rank int32 [n], biterr uint32 [n])."""
    rows = np.ascontiguousarray(type5, np.uint8)
    n, stride = rows.shape
    si = None if scramb is None else np.ascontiguousarray(scramb, np.uint32)
    n2 = N2[int(blk_type)]
    out, ok, rank, be = np.zeros((n, n2), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    rc = lib().list_emul_rows(int(blk_type), _p(rows), n, stride, _p(si), _p(out), n2, _p(ok), _p(rank), _p(be), int(route), int(T), int(bits_rescue))
    assert rc == 0, rc
    return out, ok, rank, be


def decode_frames(tpsap, blk_num, frames_packed, frame_type, row_frame, frame_scramb, out_stride, T):
    """The frame launch with ranks, one job of a coded kind -> (rows [n][out_stride], crc_ok, rank, biterr)."""
    fr = np.ascontiguousarray(frames_packed, np.uint32)
    ft = np.ascontiguousarray(frame_type, np.int32)
    rf = np.ascontiguousarray(row_frame, np.int32)
    sc = None if frame_scramb is None else np.ascontiguousarray(frame_scramb, np.uint32)
    n = rf.size
    out, ok, rank, be = np.zeros((n, out_stride), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    rc = lib().list_emul_frames(int(tpsap), int(blk_num), _p(fr), _p(ft), _p(rf), n, _p(sc), _p(out), out_stride, _p(ok), _p(rank), _p(be), int(T))
    if rc:
        raise ValueError("refused")
    return out, ok, rank, be


def decode_soft_rows(kind, soft_rows, scramb, T, ring=1024, bitnum=None):
    """The soft frame launch with ranks, a lane per row; the rows are laid into rings (one per row) at bit numbers that make them wrap
    -> (type-2 bits [n][type2], crc_ok, rank, biterr)."""
    tpsap, blk, train, pieces = KINDS[kind]
    rows = np.ascontiguousarray(soft_rows, np.int8)
    n = len(rows)
    rings, bn = lay_rings(kind, rows, ring, bitnum)
    ft = np.full(n, train, np.int32)
    sc = None if scramb is None else np.ascontiguousarray(scramb, np.uint32)
    n2 = TYPE2_BITS[kind]
    out, ok, rank, be = np.zeros((n, n2), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    rc = lib().list_emul_soft(tpsap, blk, _p(rings), ring, _p(bn), _p(ft), n, _p(sc), _p(out), n2, _p(ok), _p(rank), _p(be), int(T))
    assert rc == 0, rc
    return out, ok, rank, be
