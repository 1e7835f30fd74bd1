"""Builds and binds tests/emul/lmac_tch_soft_emul.cpp (host build of the soft-decision data channels' lane code, csrc/tch_soft_core.hpp,
behind its byte-row and ring front ends)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib
from tests.soft_pipeline import lay_rings

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_tch_soft_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "lmac_tch_soft_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + \
    [os.path.join(CSRC, f) for f in ("tch_soft_core.hpp", "tch_core.hpp", "soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]
TCH_4_8, TCH_2_4 = 9, 10
TYPE2 = {TCH_4_8: 292, TCH_2_4: 148}
TRAIN_NORM_1 = 0

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_tch_soft_emul.cpp"], DEPS,
                         force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "tch_soft_emul_rows": (i32, [i32, vp, i32, i32, vp, vp, i32, vp]),
            "tch_soft_emul_frames": (i32, [i32, vp, C.c_uint32, vp, vp, i32, vp, vp, i32, vp]),
        })
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def decode_rows(kind, soft5, scramb, biterr=True):
    """k_tch_rows_soft's lane code, a 64-row workgroup at a time: soft5 int8 [n][in_stride] -> (rows [n][type2], biterr uint32 [n] or None)."""
    rows = np.ascontiguousarray(soft5, np.int8)
    n, stride = rows.shape
    si = np.ascontiguousarray(scramb, np.uint32)
    n2 = TYPE2[int(kind)]
    out = np.zeros((n, n2), np.uint8)
    be = np.zeros(n, np.uint32) if biterr else None
    rc = lib().tch_soft_emul_rows(int(kind), _p(rows), n, stride, _p(si), _p(out), n2, _p(be))
    assert rc == 0
    return out, be


def decode_rings(kind, soft5, scramb, biterr=True, ring=1024, bitnum=None, frame_type=None):
    """k_tch_frames_soft's lane code, one job: every row laid into a ring of its own at the SCH/F burst positions behind bit number
    bitnum[j] (None: spread so that rows wrap their ring at every offset), the rest of the ring junk; frame_type None: NORM_1 bursts.
    -> (rows [n][type2], biterr or None)."""
    rows = np.ascontiguousarray(soft5, np.int8)
    n = len(rows)
    rings, bn = lay_rings("schf", rows, ring, bitnum)
    ft = np.full(n, TRAIN_NORM_1, np.int32) if frame_type is None else np.ascontiguousarray(frame_type, np.int32)
    si = np.ascontiguousarray(scramb, np.uint32)
    n2 = TYPE2[int(kind)]
    out = np.zeros((n, n2), np.uint8)
    be = np.zeros(n, np.uint32) if biterr else None
    rc = lib().tch_soft_emul_frames(int(kind), _p(rings), ring, _p(bn), _p(ft), n, _p(si), _p(out), n2, _p(be))
    assert rc == 0
    return out, be
