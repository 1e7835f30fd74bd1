"""Writes tests/golden/lmac_tch_nblk_golden.npz: the pools and window tables of tests/tch_nblk_definition.py with the definition's
decoding and count word of every window, hard and soft, for machines without oracle/_ref.  Data only; needs
oracle/_ref/libtetra_lmac_ref.so (oracle/build_ref.sh).

    python tests/golden/make_lmac_tch_nblk_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_binding  # noqa: E402
from tests import tch_nblk_definition as nd  # noqa: E402


def make(L):
    """every array of the file, as load_golden returns them"""
    z = nd.make_inputs(L)
    z.update(nd.expected(L, z))
    return z


def main():
    z = make(ref_binding.lmac_lib())
    for k in nd.PACKED:                      # plain-bit arrays are stored packed (what load_golden unpacks)
        z[k + "_cols"] = np.int32(z[k].shape[1])
        z[k] = np.packbits(z[k], axis=1)
    np.savez_compressed(nd.GOLDEN, **z)
    print(nd.GOLDEN, os.path.getsize(nd.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
