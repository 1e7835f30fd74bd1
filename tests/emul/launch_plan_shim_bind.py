"""ctypes binding of tests/emul/launch_plan_shim.cpp (the product's launch plan, csrc/launch_plan.hpp, built for the host; TEST TOOL)."""
import ctypes as C
import os

from oracle import hostlib

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
_CSRC = os.path.join(_ROOT, "sdrpp-tetra-demodulator_amd", "csrc")
_SO = os.path.join(_HERE, "liblaunch_plan_shim.so")
_lib = None


def build():
    return hostlib.build(_SO, ["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "launch_plan_shim.cpp", "-o", hostlib.OUT],
                         [os.path.join(_HERE, "launch_plan_shim.cpp")] + [os.path.join(_CSRC, f) for f in ("launch_plan.hpp", "design.hpp", "demod_core.hpp")])


def plan(n_channels, cus, flags, samplerate=-1.0, rrc_tap_count=-1):
    """host::plan_launch for a fresh handle of these parameters: dict(generic, n_wide, rest_ch, deep, long_rows, lanes), None if refused."""
    global _lib
    if _lib is None:
        _lib = hostlib.load(build(), {"launch_plan_shim": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_int)])})
    out = (C.c_int * 6)()
    if _lib.launch_plan_shim(n_channels, cus, flags, samplerate, rrc_tap_count, out) != 0:
        return None
    return dict(zip(("generic", "n_wide", "rest_ch", "deep", "long_rows", "lanes"), list(out)))
