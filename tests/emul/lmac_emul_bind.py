"""Builds and binds tests/emul/lmac_emul.cpp (host build of the lower-MAC decoder's lane-level code)."""
import ctypes as C
import os

import numpy as np

from oracle import hostlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(HERE, "liblmac_emul.so")
DEPS = [os.path.join(HERE, "lmac_emul.cpp"), os.path.join(HERE, "lmac_lane_io.hpp"),
        os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "lmac_core.hpp"),
        os.path.join(ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "demux_core.hpp")]

_lib = None


def build(force=False):
    return hostlib.build(LIB, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", hostlib.OUT, "lmac_emul.cpp"], DEPS, force=force)


def lib():
    global _lib
    if _lib is None:
        vp, i32 = C.c_void_p, C.c_int
        _lib = hostlib.load(build(), {
            "lmac_emul_decode_route": (i32, [i32, i32, i32, i32, vp, i32, i32, vp, vp, i32, vp, i32, C.POINTER(C.c_int32)]),
            "lmac_emul_decode_frames": (i32, [i32, i32, vp, vp, vp, i32, vp, vp, i32, vp]),
            "lmac_emul_tdma_advance": (None, [vp, i32, i32, vp]),
            "lmac_emul_track": (None, [vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32]),
            "lmac_emul_stage": (None, [i32, vp, i32, i32, vp, vp]),
            "lmac_emul_unit_row": (None, [i32, i32, vp]),
            "lmac_emul_sequence": (C.c_uint32, [i32, C.c_uint32, vp]),
            "lmac_emul_blk_param": (i32, [i32, vp]),
        })
    return _lib


def blk_param(blk_type):
    """blk_param(type) of lmac_core.hpp, the table the kernels use: (type345, type2, type1, a, crc)."""
    v = np.zeros(5, np.int32)
    assert lib().lmac_emul_blk_param(int(blk_type), v.ctypes.data_as(C.c_void_p)) == 0
    return tuple(int(x) for x in v)


def __getattr__(name):
    # BLK_PARAM: the coded kinds' (type345, type2, type1, a), read from the library on first use
    if name == "BLK_PARAM":
        globals()[name] = {t: blk_param(t)[:4] for t in (0, 1, 2, 4, 5)}
        return globals()[name]
    raise AttributeError(name)


def decode_route(blk_type, type5, scramb, route=0, out_stride=None, fill=0):
    """k_lmac_decode's lane code, a 64-row workgroup at a time (route 1: the byte route forced), into rows of out_stride bytes pre-filled
    with `fill` -> (rows [n][out_stride], crc_ok, fast_rows = the rows of the workgroups that took the packed route)."""
    n345, n2, n1, a, _ = blk_param(blk_type)
    rows = np.ascontiguousarray(type5, np.uint8)
    n, stride = rows.shape
    si = np.ascontiguousarray(scramb, np.uint32)
    out = np.full((n, n2 if out_stride is None else out_stride), fill, np.uint8)
    ok = np.zeros(n, np.int32)
    fast = C.c_int32(-1)
    vp = C.c_void_p
    rc = lib().lmac_emul_decode_route(n345, n2, n1, a, rows.ctypes.data_as(vp), n, stride, si.ctypes.data_as(vp), out.ctypes.data_as(vp), out.shape[1],
                                     ok.ctypes.data_as(vp), int(route), C.byref(fast))
    assert rc == 0
    return out, ok, fast.value


def decode_batch(blk_type, type5, scramb):
    return decode_route(blk_type, type5, scramb)[:2]


def stage(blk_type, type5):
    """The cooperative front end alone: (packed words uint32 [n][14] of every row, bit i at bit 31 - (i & 31) of word i >> 5; whether the
    row's workgroup took the packed route)."""
    rows = np.ascontiguousarray(type5, np.uint8)
    xb = np.zeros((len(rows), 14), np.uint32)
    took = np.zeros(len(rows), np.int32)
    vp = C.c_void_p
    lib().lmac_emul_stage(blk_param(blk_type)[0], rows.ctypes.data_as(vp), len(rows), rows.shape[1], xb.ctypes.data_as(vp), took.ctypes.data_as(vp))
    return xb, took.astype(bool)


def sequence(type345, code):
    """lane_sequence (lmac_core.hpp) for a block of type345 bits: (the words it hands out, uint32 [14], zero where it hands out none;
    the mask of those it does)."""
    words = np.zeros(14, np.uint32)
    mask = lib().lmac_emul_sequence(int(type345), int(code) & 0xffffffff, words.ctypes.data_as(C.c_void_p))
    return words, int(mask)


def unit_row(units, n):
    """unit_row(i, unit_inverse(units)) of lmac_core.hpp for i = 0 .. n - 1: the multiply-shift i // units of the front end and the write-back."""
    out = np.zeros(n, np.int32)
    lib().lmac_emul_unit_row(int(units), int(n), out.ctypes.data_as(C.c_void_p))
    return out


def decode_frames(tpsap, blk_num, frames_packed, frame_type, row_frame, frame_scramb, out_stride):
    """The lane code of k_lmac_frames (tetra_lmac_decode_frames_device, one job) for the listed frames: (rows [n][out_stride], crc_ok)."""
    fr = np.ascontiguousarray(frames_packed, np.uint32)
    ft = np.ascontiguousarray(frame_type, np.int32)
    rf = np.ascontiguousarray(row_frame, np.int32)
    sc = None if frame_scramb is None else np.ascontiguousarray(frame_scramb, np.uint32)
    out = np.zeros((rf.size, out_stride), np.uint8)
    ok = np.zeros(rf.size, np.int32)
    vp = C.c_void_p
    rc = lib().lmac_emul_decode_frames(int(tpsap), int(blk_num), fr.ctypes.data_as(vp), ft.ctypes.data_as(vp), rf.ctypes.data_as(vp), rf.size,
                                      None if sc is None else sc.ctypes.data_as(vp), out.ctypes.data_as(vp), out_stride, ok.ctypes.data_as(vp))
    if rc:
        raise ValueError("refused")
    return out, ok


def tdma_advance(start, kmax):
    """tdma_advance (lmac_core.hpp) built for the host: start [n][3] (tn, fn, mn) -> [n][kmax] packed times after k = 1..kmax steps."""
    st = np.ascontiguousarray(start, np.uint32)
    out = np.zeros((len(st), kmax), np.uint32)
    vp = C.c_void_p
    lib().lmac_emul_tdma_advance(st.ctypes.data_as(vp), len(st), int(kmax), out.ctypes.data_as(vp))
    return out


def track(sb1_type2, crc_ok, valid, n_frames, cell, stale_tcd_on_bad_crc=False):
    """k_track's rule (lmac_core.hpp track_slot / track_carry) built for the host, slot layout: sb1_type2 [n_channels * F][stride] decoded
    SB1 rows, crc_ok / valid per frame slot, n_frames [n_channels] consumed frames (None: all), cell [n_channels][10] uint32
    (tetra_lmac_cell_state_t) updated in place -> (code, time on entry, time after the SB1) per frame slot.  stale_tcd_on_bad_crc plants
    the tracker's earlier rule (a bad-CRC SB1 sets the clock to the last good SYNC PDU's time): for tests that show they would notice."""
    rows = np.ascontiguousarray(sb1_type2, np.uint8)
    n_ch = len(cell)
    F = rows.shape[0] // n_ch
    assert cell.dtype == np.uint32 and cell.flags.c_contiguous and cell.shape == (n_ch, 10) and rows.shape[1] >= 56
    ok, va = np.ascontiguousarray(crc_ok, np.int32), np.ascontiguousarray(valid, np.int32)
    nf = None if n_frames is None else np.ascontiguousarray(n_frames, np.int32)
    outs = [np.zeros(n_ch * F, np.uint32) for _ in range(3)]
    vp = C.c_void_p
    lib().lmac_emul_track(rows.ctypes.data_as(vp), int(rows.shape[1]), ok.ctypes.data_as(vp), va.ctypes.data_as(vp),
                         None if nf is None else nf.ctypes.data_as(vp), n_ch, F, cell.ctypes.data_as(vp), *(o.ctypes.data_as(vp) for o in outs),
                         int(bool(stale_tcd_on_bad_crc)))
    return tuple(outs)
