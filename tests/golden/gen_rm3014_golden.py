"""Generates tests/golden/rm3014_codewords.npy: tetra_rm3014_compute(v) of the REFERENCE for all 16 384 information words v, as uint32
(information bits in bits 29..16, parity in 15..0).  The reference's lower_mac/tetra_rm3014.c is compiled where it lies into a
temporary directory outside the repository and called through ctypes; only the recorded values are kept.  Data only; run in the build
container, where the reference is present:
    python tests/golden/gen_rm3014_golden.py [path of the reference checkout]"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rm3014_codewords.npy")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TETRA_REFERENCE", "/root/reference")
    src_dir = os.path.join(ref, "src", "decoder", "src")
    src = os.path.join(src_dir, "lower_mac", "tetra_rm3014.c")
    if not os.path.exists(src):
        raise SystemExit("reference source not found: " + src)
    with tempfile.TemporaryDirectory() as td:
        lib = os.path.join(td, "librm3014_ref.so")
        subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I", src_dir, "-o", lib, src], check=True)
        L = C.CDLL(lib)
        L.tetra_rm3014_init.restype = None
        L.tetra_rm3014_compute.argtypes = [C.c_uint16]
        L.tetra_rm3014_compute.restype = C.c_uint32
        L.tetra_rm3014_init()
        words = np.array([L.tetra_rm3014_compute(v) for v in range(1 << 14)], np.uint32)
    assert (words >> 16 == np.arange(1 << 14)).all(), "systematic: the information bits are bits 29..16"
    np.save(OUT, words)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
