"""Builds and binds tests/emul/lmac_soft_emul.cpp (host build of the soft-decision option's lane code, csrc/soft_core.hpp)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib
from tests.soft_pipeline import KINDS, TYPE2_BITS, lay_rings  # noqa: F401 (the kinds' tables: also imported from here)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_soft_emul.so")
CSRC = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
DEPS = [os.path.join(HERE, "lmac_soft_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp")] + [os.path.join(CSRC, f) for f in ("soft_core.hpp", "lmac_core.hpp", "demux_core.hpp")]

_lib = None


def build(force=False):
    # -ffp-contract=off: the quantiser's separate multiplies and adds, as the library's flags have them
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_soft_emul.cpp"], DEPS,
                         force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "soft_emul_q": (i32, []),
            "soft_emul_g": (C.c_float, []),
            "soft_emul_fresh_prev": (C.c_float, []),
            "soft_emul_ring_size": (C.c_uint32, [i32]),
            "soft_emul_quantise": (None, [vp, i32, vp, vp]),
            "soft_emul_decode": (i32, [i32, i32, vp, C.c_uint32, vp, vp, i32, vp, vp, i32, vp]),
        })
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def Q():
    return int(lib().soft_emul_q())


def G():
    return float(lib().soft_emul_g())


def fresh_prev():
    return np.float32(lib().soft_emul_fresh_prev())


def ring_size(bits_stride):
    return int(lib().soft_emul_ring_size(int(bits_stride)))


def quantise(sym, prev=None):
    """k_soft's lane code for one channel: sym complex64 [n] after `prev` (None: a fresh channel) -> (int8 [2n], the new prev)."""
    z = np.ascontiguousarray(sym, np.complex64)
    pv = np.array([fresh_prev()] * 2 if prev is None else [prev.real, prev.imag], np.float32)
    out = np.zeros(2 * z.size, np.int8)
    lib().soft_emul_quantise(_p(z), z.size, _p(pv), _p(out))
    return out, np.complex64(complex(pv[0], pv[1]))


def decode_rows(kind, soft_rows, scramb=None, ring=1024, bitnum=None):
    """One lane of k_lmac_frames_soft per row.  soft_rows int8 [n][type-5 bits of the kind]: every row is laid into a ring of its own at
    the kind's burst positions behind bit number bitnum[j] (None: spread so that rows wrap their ring at every offset), the rest of
    the ring filled with junk.  -> (type-2 bits uint8 [n][type2], crc_ok int32 [n])."""
    tpsap, blk, train, pieces = KINDS[kind]
    rows = np.ascontiguousarray(soft_rows, np.int8)
    n = len(rows)
    rings, bn = lay_rings(kind, rows, ring, bitnum)
    ft = np.full(n, train, np.int32)
    sc = None if scramb is None else np.ascontiguousarray(scramb, np.uint32)
    n2 = TYPE2_BITS[kind]
    out, ok = np.zeros((n, n2), np.uint8), np.zeros(n, np.int32)
    rc = lib().soft_emul_decode(tpsap, blk, _p(rings), ring, _p(bn), _p(ft), n, None if sc is None else _p(sc), _p(out), n2, _p(ok))
    assert rc == 0
    return out, ok
