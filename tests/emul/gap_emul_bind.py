"""Builds and binds tests/emul/gap_emul.cpp: the host build of the stream gap's arithmetic (csrc/handover_core.hpp's anchor and planting
rule; include/ext/tetra_gap.h).  The restart and the ASSIST state a resumed channel runs in are handover_emul_bind's: Bank here is that
module's with anchor() beside resume().  TEST TOOL."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib
from tests.emul import handover_emul_bind as H
from tests.emul.handover_emul_bind import (ASSIST_FIELDS, CELL_FIELDS, EXPIRED, LOCKED, NONE, PENDING, REFUSED, ST_ASSIST, ST_KNOW_FSTART,  # noqa: F401
                                           ST_LOCKED, ST_UNLOCKED, own_donor_vs_resume, tdma_steps)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
LIB = os.path.join(HERE, "libgap_emul.so")
DEPS = [os.path.join(HERE, "gap_emul.cpp")] + \
       [os.path.join(CSRC, f) for f in ("bsync_core.hpp", "handover_core.hpp", "lmac_core.hpp", "demux_core.hpp", "retune_core.hpp")]

_lib = None


def build(force=False):
    H.build(force=force)
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "gap_emul.cpp"], DEPS, force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "gap_emul_tdma_period": (i32, []),
            "gap_emul_expect": (i32, [C.c_int32, C.c_uint32, i32, vp]),
            "gap_emul_anchor": (i32, [vp, vp, vp, i32, vp, vp]),
        })
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def tdma_period():
    return int(lib().gap_emul_tdma_period())


def expect(d, elapsed, window):
    """-> (expect, m) of the rule for d = Rcv - a and `elapsed` bits."""
    m = np.zeros(1, np.int32)
    e = lib().gap_emul_expect(int(d), int(elapsed), int(window), _p(m))
    return int(e), int(m[0])


class Bank(H.Bank):
    """handover_emul_bind.Bank with the anchor a resume() plants from."""

    def anchor(self, c):
        """-> (ok, d, (tn, fn, mn))"""
        d, q = np.zeros(1, np.int32), np.zeros(3, np.uint32)
        ok = lib().gap_emul_anchor(_p(self.st), _p(self.assist), _p(self.cell), int(c), _p(d), _p(q))
        return int(ok), int(d[0]), tuple(int(x) for x in q)
