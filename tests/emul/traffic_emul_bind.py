"""Builds and binds tests/emul/traffic_emul.cpp: the host build of the traffic routing's lane code (csrc/traffic_core.hpp;
include/ext/tetra_traffic.h).  TEST TOOL."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "libtraffic_emul.so")
DEPS = [os.path.join(HERE, "traffic_emul.cpp"), os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "traffic_core.hpp")]

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "traffic_emul.cpp"], DEPS, force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "traffic_emul_kinds": (i32, []),
            "traffic_emul_slot_valid": (i32, [i32, i32]),
            "traffic_emul_route": (None, [i32, vp, vp, vp, vp, vp, vp, i32, vp]),
            "traffic_emul_lists": (None, [i32, vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]),
        })
        assert _lib.traffic_emul_kinds() == 3
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def slot_valid(kind, usage):
    return bool(lib().traffic_emul_slot_valid(int(kind), int(usage)))


def route(frame_type, scramb, time, slots, bbk_ok, bbk_bits):
    """The rule per entry: frame_type / scramb / time / bbk_ok [n], slots uint8 [n][4][4] (kind, usage, pad, pad), bbk_bits uint8
    [n][>= 8] -> int32 [n]: the TCH kind 8 / 9 / 10, or 0."""
    ft, sc, t, ok = (np.ascontiguousarray(a, d) for a, d in ((frame_type, np.int32), (scramb, np.uint32), (time, np.uint32), (bbk_ok, np.int32)))
    s, b = np.ascontiguousarray(slots, np.uint8), np.ascontiguousarray(bbk_bits, np.uint8)
    n = ft.size
    assert s.shape == (n, 4, 4) and b.shape[0] == n and b.shape[1] >= 8 and sc.size == t.size == ok.size == n
    out = np.zeros(n, np.int32)
    lib().traffic_emul_route(n, _p(ft), _p(sc), _p(t), _p(s), _p(ok), _p(b), b.shape[1], _p(out))
    return np.where(out < 0, 0, out + 8)


def lists(any_list, F, frame_type, scramb, time, table, bbk_ok, bbk_t2, max_rows):
    """One call as the three kernels leave it: any_list int32 [n] (frames; entry j is BBK row j), per-frame arrays [C * F], table uint8
    [C][4][4], bbk_t2 uint8 [n][stride] -> ({kind: the kept frames}, {kind: (routed, kept, dropped)})."""
    al, ft, sc, t, ok = (np.ascontiguousarray(a, d) for a, d in ((any_list, np.int32), (frame_type, np.int32), (scramb, np.uint32), (time, np.uint32),
                                                                  (bbk_ok, np.int32)))
    tab, b = np.ascontiguousarray(table, np.uint8), np.ascontiguousarray(bbk_t2, np.uint8).reshape(max(al.size, 1), -1)
    out, counts = np.full((3, max_rows), -1, np.int32), np.zeros((3, 3), np.int32)
    lib().traffic_emul_lists(al.size, _p(al), int(F), _p(ft), _p(sc), _p(t), _p(tab), _p(ok), _p(b), b.shape[1], int(max_rows), _p(out), _p(counts))
    return {8 + k: out[k, :counts[k, 1]].copy() for k in range(3)}, {8 + k: tuple(int(v) for v in counts[k]) for k in range(3)}
