"""Writes tests/golden/lmac_tch_golden.npz: the row sets of tests/tch_definition.py with the reference's decoding of every row and the
definition's bit-error words, for machines without oracle/_ref.  Data only; needs oracle/_ref/libtetra_lmac_ref.so (oracle/build_ref.sh).

    python tests/golden/make_lmac_tch_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_binding  # noqa: E402
from tests import tch_definition as td  # noqa: E402


def main():
    L = ref_binding.lmac_lib()
    z = td.make_inputs(L)
    z.update(td.expected(L, z))
    # plain-bit inputs are stored packed (what load_golden unpacks)
    for k in ("bits",) + tuple("%s_%d" % (s, kind) for kind in td.CODED for s in ("clean", "noisy", "pay")):
        z[k + "_cols"] = np.int32(z[k].shape[1])
        z[k] = np.packbits(z[k], axis=1)
    np.savez_compressed(td.GOLDEN, **z)
    print(td.GOLDEN, os.path.getsize(td.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
