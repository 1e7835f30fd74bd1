"""ctypes binding of tests/emul/rx_out_ext_emul.cpp (host build of the extras writer's lane code in csrc/rx_out_core.hpp; TEST TOOL)."""
import ctypes as C
import os

from oracle import hostlib

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_SO = os.path.join(_HERE, "librx_out_ext_emul.so")
_lib = None


def build():
    inc = os.path.join(_ROOT, "include")
    return hostlib.build(_SO, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "rx_out_ext_emul.cpp", "-o", hostlib.OUT],
                         [os.path.join(_HERE, "rx_out_ext_emul.cpp"), os.path.join(_ROOT, "sdrpp-tetra-demodulator_amd", "csrc", "rx_out_core.hpp"),
                          os.path.join(inc, "tetra_rx_out.h"), os.path.join(inc, "ext", "tetra_rx_out_ext.h")])


def lib():
    global _lib
    if _lib is None:
        vp, i32, u64 = C.c_void_p, C.c_int, C.c_uint64
        _lib = hostlib.load(build(), {
            "rx_out_ext_emul_column": (None, [vp, i32, i32, i32, vp, i32, i32, u64, i32, vp]),
            "rx_out_ext_emul_table": (None, [vp, u64, i32, vp]),
            "rx_out_ext_emul_layout": (u64, [vp, vp, i32, i32, i32, i32, vp, vp]),
            "rx_out_ext_emul_snap_offset": (u64, [i32, i32]),
        })
    return _lib
