"""Writes tests/golden/rx_options_golden.npz: what the host pipeline of tests/options_pipeline.py gives for its stream under the 20 row
classes of the receive chain's create flags (synchroniser rule x hard / soft x list decoding x AACH rule) -- the oracle demodulator's bits,
the coded rows once per (synchroniser, soft, list), the AACH rows per class, the final cells and the miss counters.  Needs oracle/_ref
(the tolerant synchroniser's restatement searches with the reference's tetra_find_train_seq).

    python tests/golden/make_rx_options_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make():
    """-> (the oracle demodulator's bits per channel, {class flags: expectation}) from oracle/_ref"""
    import tetra_amd
    from oracle import binding as ob, ref_binding as ref
    from tests import options_pipeline as OP
    from tests import soft_pipeline as sp
    ob.build()
    bits, soft = sp.oracle_streams(ob, OP.stream_iq(tetra_amd.pkg.synth))
    return bits, OP.expectations(ref, ob, bits, soft)


def main():
    from tests import options_pipeline as OP
    bits, want = make()
    np.savez_compressed(OP.GOLDEN, **OP.to_arrays(bits, want))
    assert OP.same(OP.load_golden(), (bits, want))
    print({OP.class_name(f): len(w["rows"]) for f, w in want.items()}, os.path.getsize(OP.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
