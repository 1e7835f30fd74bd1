"""Generates tests/golden/chan_emul_unshifted.npz and tests/golden/resamp_emul.npz: what the host emulations of the wideband front
end (tests/emul/chan_emul.cpp, tests/emul/resamp_emul.cpp) computed BEFORE the shifted channeliser emulation and the selecting
resampler emulation were folded into them.  The committed files were recorded at that parent commit, with ResampSelectEmul still
in its own library; they pin the merged emulations to the earlier ones bit for bit (tests/test_chan_shift.py,
tests/test_resamp.py).  Neither path calls libm, so the rows are reproducible: run this again only to add a case.

Channeliser: the un-shifted lane code, three sample formats, P = 4, 6, 8, with the seeds and cuts of
tests/test_chan_shift.py's shift-zero test; of the 17 output frames of a case the first and last of every call are kept.
Resampler: one case per kernel wrapper, input and prototype stored with the output.
Run from the repo root:  python tests/golden/make_front_end_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import binding as ob  # noqa: E402
from tests import test_chan_shift as TS  # noqa: E402
from tests.emul import chan_emul_bind as ce  # noqa: E402
from tests.emul import resamp_emul_bind as re_  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CHAN_KEEP = [0, 1, 7, 8, 16]          # frames of the concatenated output: first and last of the calls that emit 1, 7 and 9 frames
RESAMP_CUTS = [0, 0, 1, 3, 24, 27, 40, 41, 90]
RESAMP_COLS = [7, 2, 9]
# name -> (I, DN, T, W or None for picked columns, generic)
RESAMP_CASES = {"full_w4": (18, 25, 16, 4, False), "full_w2": (18, 25, 16, 2, False), "full_generic_w4": (5, 7, 11, 4, True),
                "full_generic_w2": (5, 7, 11, 2, True), "pick": (18, 25, 16, None, False), "pick_generic": (5, 7, 11, None, True)}


def chan():
    out = {"keep": np.array(CHAN_KEEP), "cuts": np.array(TS.SHIFT_ZERO_CUTS)}
    for dtype in (np.complex64, np.int16, np.int8):
        for P, x in TS.shift_zero_inputs(dtype):
            em = ce.ChanFftEmul(P, ob.ChanOracle(800, P, 400).h)
            y = np.concatenate([em.process(x[a:b]) for a, b in zip(TS.SHIFT_ZERO_CUTS, TS.SHIFT_ZERO_CUTS[1:])])
            assert y.shape == (17, 800)
            out["%s_P%d" % (np.dtype(dtype).name, P)] = y[CHAN_KEEP]
    np.savez(os.path.join(HERE, "chan_emul_unshifted.npz"), **out)


def resamp():
    rng = np.random.default_rng(19)
    C = 10
    x = (rng.standard_normal((RESAMP_CUTS[-1], C)) + 1j * rng.standard_normal((RESAMP_CUTS[-1], C))).astype(np.complex64)
    out = {"x": x, "cuts": np.array(RESAMP_CUTS), "cols": np.array(RESAMP_COLS, np.int32)}
    for name, (I, DN, T, W, generic) in RESAMP_CASES.items():
        proto = ob.ResampOracle(C, I, DN, T).h
        if W is None:
            em = re_.ResampSelectEmul(C, RESAMP_COLS, I, DN, T, proto, generic=generic)
        else:
            em = re_.ResampEmul(C, I, DN, T, proto, generic=generic, W=W)
        out[name + "_case"] = np.array([I, DN, T, W or 0, int(generic)])
        out[name + "_proto"] = proto
        out[name] = np.concatenate([em.process(x[a:b]) for a, b in zip(RESAMP_CUTS, RESAMP_CUTS[1:])])
    np.savez(os.path.join(HERE, "resamp_emul.npz"), **out)


if __name__ == "__main__":
    ob.build()
    chan()
    resamp()
