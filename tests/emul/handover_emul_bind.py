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
DEPS = [os.path.join(HERE, f) for f in ("handover_emul.cpp", "bsync_lane_io.hpp", "restart_lanes.hpp")] + \
       [os.path.join(CSRC, f) for f in ("bsync_core.hpp", "handover_core.hpp", "lmac_core.hpp", "demux_core.hpp", "retune_core.hpp")]

ST_ASSIST, ST_LOCKED, ST_KNOW_FSTART, ST_UNLOCKED = 3, 2, 1, 0
NONE, PENDING, LOCKED, EXPIRED, REFUSED = range(5)
# bsync_core::Assist, word for word
ASSIST_FIELDS = ("status", "waited", "offset", "expect", "window", "slots_left", "result", "reserved")
CELL_FIELDS = ("scramb_init", "colour_code", "mcc", "mnc", "tcd_tn", "tcd_fn", "tcd_mn", "phy_tn", "phy_fn", "phy_mn")
LINK_WORDS = 6                                     # tetra_rx_link_t

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
            "handover_emul_restart": (None, [vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, C.c_uint32, i32, i32]),
            "handover_emul_own_donor_vs_resume": (C.c_longlong, [vp, i32, i32, vp, i32, vp, vp]),
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


def own_donor_vs_resume(cell, max_bits, max_window, max_slots):
    """A LOCKED channel with `cell` restarted as the heir of itself as a donor and as its own heir after no gap, for every bits_in_buf
    0 .. max_bits x window 0 .. max_window x max_slots -> (cases that differ in State, Assist or cell, cases planted, the first that differs)."""
    cell, ms = np.array(cell, np.uint32), np.array(max_slots, np.int32)
    planted, first = np.zeros(1, np.int64), np.zeros(3, np.int32)
    differing = lib().handover_emul_own_donor_vs_resume(_p(cell), int(max_bits), int(max_window), _p(ms), ms.size, _p(planted), _p(first))
    return int(differing), int(planted[0]), tuple(int(v) for v in first)


class Bank:
    """C channels as the chain keeps them: synchroniser State [C][4], bit buffers [C][4096], hand-over fields [C][8], cell state [C][10],
    link figures [C][6 words], miss counters [C].  tol: None = the reference's lock rule, else (tol_norm, tol_sync, max_miss).  feed() is
    one call of one channel's synchroniser; reset() / plant() / resume() are what k_restart_tail does to a channel without a source, with
    a donor and as its own heir; apply() is k_handover_apply."""

    def __init__(self, n, tol=None, use_batch=True, packed=False):
        self.n, self.packed, self.use_batch = n, bool(packed), int(bool(use_batch))
        self.tol = None if tol is None else np.array(tol, np.int32)
        self.st = np.zeros((n, 4), np.uint32)
        self.carry = np.zeros((n, 4096), np.uint8)
        self.assist = np.zeros((n, len(ASSIST_FIELDS)), np.int32)
        self.cell = np.zeros((n, len(CELL_FIELDS)), np.uint32)
        self.link = np.zeros((n, LINK_WORDS), np.uint32)
        self.miss = np.zeros(n, np.int32)

    def restart(self, c, src=-1, accept_pending=False, elapsed=0, window=0, max_slots=0):
        lib().handover_emul_restart(_p(self.st), _p(self.carry), _p(self.cell), _p(self.link), LINK_WORDS, _p(self.miss), _p(self.assist), int(c), int(src),
                                    int(accept_pending), int(elapsed), int(window), int(max_slots))

    def reset(self, c):
        self.restart(c)

    def plant(self, c, donor, window, max_slots):
        self.restart(c, donor, False, 0, window, max_slots)

    def resume(self, c, elapsed, window, max_slots):
        self.restart(c, c, True, elapsed, window, max_slots)

    def apply(self):
        lib().handover_emul_apply(_p(self.assist), _p(self.cell), self.n)

    def field(self, c, name):
        return int(self.assist[c, ASSIST_FIELDS.index(name)])

    def status(self, c):
        return tuple(int(v) for v in self.assist[c, :3])

    def state(self, c):
        return tuple(int(v) for v in self.st[c])

    def feed_in_cuts(self, c, stream, cut):
        """`stream` through channel c in calls of `cut` bits ("ragged": a fixed mix of sizes), the apply step behind each -> (frames, types,
        bit numbers, the result words in their order, the final State, hand-over fields, cell, bit buffer and miss counter)"""
        r = np.random.default_rng(99)
        at, frames, types, nums, results = 0, [], [], [], []
        while at < stream.size:
            n = int(r.choice((1, 3, 200, 509, 511, 777, 2040))) if cut == "ragged" else cut
            fr, ty, bn = self.feed(c, stream[at:at + n])
            at += n
            frames += [f.tobytes() for f in fr]
            types += list(ty)
            nums += list(bn)
            if self.field(c, "result"):
                results.append(self.field(c, "result"))
            self.apply()
        return frames, types, nums, results, self.state(c), tuple(self.assist[c]), tuple(self.cell[c]), self.carry[c][:self.state(c)[1]].tobytes(), int(self.miss[c])

    def feed(self, c, bits):
        b = np.ascontiguousarray(bits, np.uint8)
        cap = (4096 + b.size) // 510 + 4
        fr = np.zeros((cap, 16), np.uint32) if self.packed else np.zeros((cap, 512), np.uint8)
        ty, bn = np.zeros(cap, np.int32), np.zeros(cap, np.uint32)
        n = lib().handover_emul_process(_p(self.st[c]), _p(self.assist[c]), _p(self.miss[c:c + 1]), _p(self.carry[c]), _p(b), b.size,
                                        None if self.tol is None else _p(self.tol), _p(fr), int(self.packed), _p(ty), _p(bn), cap, self.use_batch)
        assert n >= 0, n
        return (fr[:n] if self.packed else fr[:n, :510]).copy(), ty[:n].copy(), bn[:n].copy()
