"""Generates tests/golden/sync_track_golden.npz: the SYNC tracker's inputs (tests/test_sync_track.make_case: per frame slot whether a SYNC
burst is there, its SB1 block's type-5 bits, consumed frames per call, start clock) and what the REFERENCE's own tp_sap_udata_ind recorded
for them (run_reference: oracle/_ref/libtetra_rxchain_ref.so = src/decoder/src/lower_mac/tetra_lower_mac.c behind the test-side recorder
tests/refrec/tmv_sap_recorder.c, built by oracle/build_ref.sh).  Data only; run from the repo root in the build container:
python tests/golden/make_sync_track_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_binding as R  # noqa: E402
from tests.test_sync_track import GOLDEN, GOLDEN_CASES, GOLDEN_REC_KEYS, make_case, run_reference  # noqa: E402

out = {"n_cases": np.int32(len(GOLDEN_CASES))}
for i, (seed, n_ch, F) in enumerate(GOLDEN_CASES):
    case = make_case(R, seed, n_ch, F)
    rec = run_reference(R, case)
    for k in ("valid", "follow", "nfr", "phy0"):
        out[f"{k}_{i}"] = case[k]
    out[f"t5_packed_{i}"] = np.packbits(case["t5"], axis=-1)
    for k in GOLDEN_REC_KEYS:
        out[f"{k}_{i}"] = np.packbits(rec[k], axis=-1) if k == "sb1_bits" else rec[k]
np.savez_compressed(GOLDEN, **out)
print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes", {k: np.shape(v) for k, v in out.items()})
