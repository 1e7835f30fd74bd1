"""Writes tests/golden/rx_soft_golden.npz: the rows the reference-only host pipeline (tests/soft_pipeline.py) gives for the
operating point of tests/test_rx_soft.py, with hard and with soft decisions.  Needs oracle/_ref (the reference's lower MAC).

    python tests/golden/make_rx_soft_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import tetra_amd
    from oracle import binding as ob, ref_binding as ref
    from tests import chain_host as ch
    from tests import soft_pipeline as sp
    iq = ch.operating_point(tetra_amd.pkg.synth, 11.0)[2]
    out = {}
    for name, use_soft in (("hard", False), ("soft", True)):
        rows = sp.stream_rows(ref, ob, iq, use_soft)
        for k, v in rows.items():
            for field, arr in ch.rows_to_arrays(v, ch.TYPE1_BITS[k]).items():
                out["%s_%d_%s" % (name, k, field)] = arr
        print(name, {k: (len(v), sum(r[2] for r in v)) for k, v in rows.items()})
    np.savez_compressed(ch.RX_SOFT_GOLDEN, **out)


if __name__ == "__main__":
    main()
