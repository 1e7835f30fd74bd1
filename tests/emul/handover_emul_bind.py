"""Builds and binds tests/emul/handover_emul.cpp: the host build of the hand-over's lane code (csrc/bsync_core.hpp's ASSIST state,
csrc/handover_core.hpp's planting and apply step; include/ext/tetra_handover.h).  TEST TOOL."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
LIB = os.path.join(HERE, "libhandover_emul.so")
DEPS = [os.path.join(HERE, "handover_emul.cpp"), os.path.join(HERE, "bsync_lane_io.hpp")] + \
       [os.path.join(CSRC, f) for f in ("bsync_core.hpp", "handover_core.hpp", "lmac_core.hpp", "demux_core.hpp")]

ST_ASSIST, ST_LOCKED, ST_KNOW_FSTART, ST_UNLOCKED = 3, 2, 1, 0
NONE, PENDING, LOCKED, EXPIRED, REFUSED = range(5)
# bsync_core::Assist, word for word
ASSIST_FIELDS = ("status", "waited", "offset", "expect", "window", "slots_left", "result", "reserved")
CELL_FIELDS = ("scramb_init", "colour_code", "mcc", "mnc", "tcd_tn", "tcd_fn", "tcd_mn", "phy_tn", "phy_fn", "phy_mn")

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "handover_emul.cpp"], DEPS, force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "handover_emul_assist_words": (i32, []),
            "handover_emul_process": (i32, [vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, i32]),
            "handover_emul_expect": (i32, [C.c_uint32, i32, vp]),
            "handover_emul_tdma_steps": (None, [vp, i32]),
            "handover_emul_plant": (None, [vp, vp, vp, i32, i32, i32, i32]),
            "handover_emul_apply": (None, [vp, vp, i32]),
        })
        assert _lib.handover_emul_assist_words() == len(ASSIST_FIELDS)
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def expect(bits_in_buf, window):
    m = np.zeros(1, np.int32)
    e = lib().handover_emul_expect(int(bits_in_buf), int(window), _p(m))
    return int(e), int(m[0])


def tdma_steps(t, k):
    v = np.array(t, np.uint32)
    lib().handover_emul_tdma_steps(_p(v), int(k))
    return tuple(int(x) for x in v)


class Bank:
    """C channels as the chain keeps them: synchroniser State [C][4], bit buffers [C][4096], hand-over fields [C][8], cell state [C][10],
    miss counters [C].  tol: None = the reference's lock rule, else (tol_norm, tol_sync, max_miss).  feed() is one call of one channel's
    synchroniser, reset() / plant() / apply() what the reset kernels, k_handover_plant and k_handover_apply do."""

    def __init__(self, n, tol=None, use_batch=True, packed=False):
        self.n, self.packed, self.use_batch = n, bool(packed), int(bool(use_batch))
        self.tol = None if tol is None else np.array(tol, np.int32)
        self.st = np.zeros((n, 4), np.uint32)
        self.carry = np.zeros((n, 4096), np.uint8)
        self.assist = np.zeros((n, len(ASSIST_FIELDS)), np.int32)
        self.cell = np.zeros((n, len(CELL_FIELDS)), np.uint32)
        self.miss = np.zeros(n, np.int32)

    def reset(self, c):
        for a in (self.st, self.carry, self.assist, self.cell):
            a[c] = 0
        self.miss[c] = 0

    def plant(self, c, donor, window, max_slots):
        self.reset(c)
        lib().handover_emul_plant(_p(self.st), _p(self.assist), _p(self.cell), int(c), int(donor), int(window), int(max_slots))

    def apply(self):
        lib().handover_emul_apply(_p(self.assist), _p(self.cell), self.n)

    def field(self, c, name):
        return int(self.assist[c, ASSIST_FIELDS.index(name)])

    def status(self, c):
        return tuple(int(v) for v in self.assist[c, :3])

    def state(self, c):
        return tuple(int(v) for v in self.st[c])

    def feed(self, c, bits):
        b = np.ascontiguousarray(bits, np.uint8)
        cap = (4096 + b.size) // 510 + 4
        fr = np.zeros((cap, 16), np.uint32) if self.packed else np.zeros((cap, 512), np.uint8)
        ty, bn = np.zeros(cap, np.int32), np.zeros(cap, np.uint32)
        n = lib().handover_emul_process(_p(self.st[c]), _p(self.assist[c]), _p(self.miss[c:c + 1]), _p(self.carry[c]), _p(b), b.size,
                                        None if self.tol is None else _p(self.tol), _p(fr), int(self.packed), _p(ty), _p(bn), cap, self.use_batch)
        assert n >= 0, n
        return (fr[:n] if self.packed else fr[:n, :510]).copy(), ty[:n].copy(), bn[:n].copy()
