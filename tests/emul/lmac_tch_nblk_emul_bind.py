"""Builds and binds tests/emul/lmac_tch_nblk_emul.cpp (host build of the N-block front end of the coded data channels,
csrc/tch_nblk_core.hpp, in front of the lane code of tch_core.hpp / tch_soft_core.hpp)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_tch_nblk_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "lmac_tch_nblk_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + \
    [os.path.join(CSRC, f) for f in ("tch_nblk_core.hpp", "tch_soft_core.hpp", "tch_core.hpp", "soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]
TCH_4_8, TCH_2_4 = 9, 10
TYPE2 = {TCH_4_8: 292, TCH_2_4: 148}

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_tch_nblk_emul.cpp"], DEPS,
                         force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "tch_nblk_emul_hard": (i32, [i32, i32, vp, i32, i32, vp, vp, vp, i32, vp, i32, vp, i32, vp]),
            "tch_nblk_emul_soft": (i32, [i32, i32, vp, i32, i32, vp, vp, vp, i32, vp, i32, vp]),
        })
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def decode(kind, n, pool, scramb, windows, soft=False, biterr=True, init_index=None, route=0, n_rows=None):
    """k_tch_nblk's (soft: k_tch_nblk_soft's) lane code, a 64-block workgroup at a time: pool uint8 / int8 [n_rows][in_stride], windows
    int32 [n_blocks][n] -> (rows [n_blocks][type2], count words or None, blocks that took the packed route; soft: None).  n_rows: the
    pool's size as the entry is told it (default: all of it)."""
    rows = np.ascontiguousarray(pool, np.int8 if soft else np.uint8)
    stride = rows.shape[1]
    n_rows = len(rows) if n_rows is None else int(n_rows)
    win = np.ascontiguousarray(windows, np.int32)
    assert win.ndim == 2 and win.shape[1] == n and n_rows <= len(rows)
    si = np.ascontiguousarray(scramb, np.uint32)
    ii = None if init_index is None else np.ascontiguousarray(init_index, np.int32)
    n2 = TYPE2[int(kind)]
    out = np.zeros((len(win), n2), np.uint8)
    be = np.zeros(len(win), np.uint32) if biterr else None
    if soft:
        rc = lib().tch_nblk_emul_soft(int(kind), int(n), _p(rows), n_rows, stride, _p(si), _p(ii), _p(win), len(win), _p(out), n2, _p(be))
        fast = None
    else:
        f = C.c_int32(0)
        rc = lib().tch_nblk_emul_hard(int(kind), int(n), _p(rows), n_rows, stride, _p(si), _p(ii), _p(win), len(win), _p(out), n2, _p(be), int(route),
                                      C.addressof(f))
        fast = f.value
    assert rc == 0
    return out, be, fast
