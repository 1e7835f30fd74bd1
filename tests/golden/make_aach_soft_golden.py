"""Writes tests/golden/aach_soft_golden.npz: what the reference-only host pipeline (tests/aach_soft_pipeline.py) gives for the stream of
tests/test_aach_soft_gpu.py's chain tests -- per AACH row, in the chain's order, its label (channel, bit number, the two TDMA times), the
30 descrambled hard bits (packed) and the 30 descrambled soft values.  Needs oracle/_ref (the reference's lower MAC).

    python tests/golden/make_aach_soft_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PATH = os.path.join(ROOT, "tests", "golden", "aach_soft_golden.npz")


def make():
    import tetra_amd
    from oracle import binding as ob, ref_binding as ref
    from tests import aach_soft_pipeline as P
    g = P.stream_aach(ref, ob, P.stream_iq(tetra_amd.pkg.synth))
    return dict(label=g["label"], hard=np.packbits(g["hard"], axis=1), soft=g["soft"])


def load():
    g = np.load(PATH)
    return dict(label=g["label"], hard=np.unpackbits(g["hard"], axis=1)[:, :30], soft=g["soft"])


def main():
    from tests import aach_soft_pipeline as P
    np.savez_compressed(PATH, **make())
    print(P.scores(load())[:2])


if __name__ == "__main__":
    main()
