"""Writes tests/golden/lmac_tch_soft_golden.npz: the row sets of tests/tch_soft_definition.py with the reference's soft decoding of every
row, the definition's bit-error words and the hard definition's decoding of the gain set, for machines without oracle/_ref.  Data only;
needs oracle/_ref/libtetra_lmac_ref.so (oracle/build_ref.sh).

    python tests/golden/make_lmac_tch_soft_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_binding  # noqa: E402
from tests import tch_soft_definition as sd  # noqa: E402


def make(L):
    """every array of the file, as load_golden returns them"""
    z = sd.make_inputs(L)
    z.update(sd.expected(L, z))
    return z


def main():
    z = make(ref_binding.lmac_lib())
    for kind in sd.CODED:
        for k in ("want_%d" % kind, "hard_%d" % kind, "pay_%d" % kind):        # plain-bit arrays are stored packed (what load_golden unpacks)
            z[k + "_cols"] = np.int32(z[k].shape[1])
            z[k] = np.packbits(z[k], axis=1)
    np.savez_compressed(sd.GOLDEN, **z)
    print(sd.GOLDEN, os.path.getsize(sd.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
