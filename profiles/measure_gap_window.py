"""How far the frame start a resumed slot finds lies from the one the gap rule expects: the number the gap's default window
(include/ext/tetra_gap.h, TETRA_GAP_DEFAULT_WINDOW) rests on, and the time of the gap call.  Needs a GPU: the wideband handle itself.

Per Es/N0 (11, 20, 25 dB per carrier): tests/restart_gpu.py's band (32 bins at 800 kHz; a control carrier, a traffic carrier, a carrier of
another cell, all frame-synchronous) is fed up to the first call boundary (17.6 slots); then a random number of samples is left out --
drawn uniformly from what the capture leaves room for, 0 .. 48 slot periods, so that the elapsed bits G = n_lost * 0.045 fall anywhere
between two bits and the channeliser's frame grid (16 samples) and the resampler's phase restart anywhere --, tetra_wbrx_gap is told, and
the rest of the capture follows.  The figure recorded per carrier is the offset tetra_rx_get_handover reports: found frame start -
expected frame start.  A slot that has not locked when the capture ends is counted apart.  The arithmetic for longer gaps (m up to
2^31 / 510 slots, the clock's period of 4320) is integer and is tested on the host; what a gap longer than the capture cannot show here
is the drift of the two clocks, which DESIGN.md 8.13 budgets.

The cost: the band's capture in 0.25 s calls, the time of one call enqueued alone against tetra_wbrx_gap plus that call, by events on the
stream, median of the trials.

    python profiles/measure_gap_window.py [--trials 40] [--out profiles/r23/gap_window.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "gap_window.json"))
    args = ap.parse_args()
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    from tests.restart_gpu import BIN_A, BIN_B, BIN_C, BIN_EMPTY, CALL, D_BAND, M_BAND, band_capture as _band_capture
    bins = [BIN_A, BIN_B, BIN_C, BIN_EMPTY]
    result = {"trials": args.trials, "bits_per_sample": 0.045, "by_esn0": {}}
    largest = 0
    for esn0 in (11.0, 20.0, 25.0):
        xs = _band_capture(torch, pkg.synth, esn0_db=esn0)
        L = xs.shape[0]
        rng = np.random.default_rng(int(esn0))
        offsets, waited, not_locked, refused, frac, ms_plain, ms_gap = [], [], 0, 0, [], [], []
        for t in range(args.trials):
            n_lost = int(rng.integers(0, L - CALL - 30 * 510 * 800 // 36))          # at least 30 slot periods of capture behind the gap
            wb = pkg.WidebandRx(bins, n_channels=M_BAND, decimation=D_BAND, max_in=CALL)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            wb.process_device(xs[:CALL], CALL)
            wb.rx.wait()
            at = CALL + n_lost
            ev[0].record()
            if t % 2:                                  # every other trial times the plain call: the same samples, nobody told
                wb.process_device(xs[at:at + CALL], min(CALL, L - at))
                ev[1].record()
                wb.rx.wait()
                ms_plain.append(ev[0].elapsed_time(ev[1]))
                wb.close()
                continue
            g = wb.gap(n_lost)
            wb.process_device(xs[at:at + CALL], min(CALL, L - at))
            ev[1].record()
            wb.rx.wait()
            ms_gap.append(ev[0].elapsed_time(ev[1]))
            for a in range(at + CALL, L, CALL):
                wb.process_device(xs[a:a + CALL], min(CALL, L - a))
            frac.append(n_lost * 0.045 - g)
            for state, k, off in wb.handover_status()[:3]:
                if state == 2:
                    offsets.append(off)
                    waited.append(k)
                elif state == 4:
                    refused += 1
                else:
                    not_locked += 1
            wb.close()
        vals, counts = np.unique(np.array(offsets, np.int64), return_counts=True)
        big = int(np.abs(offsets).max()) if offsets else 0
        largest = max(largest, big)
        result["by_esn0"]["%g" % esn0] = {
            "carriers_resumed": len(offsets) + not_locked + refused, "locked": len(offsets), "not_locked_at_the_end": not_locked,
            "refused_not_locked_at_the_gap": refused, "histogram": {str(int(v)): int(c) for v, c in zip(vals, counts)}, "largest_magnitude": big,
            "slot_periods_waited_max": int(max(waited)) if waited else None, "slot_periods_waited_mean": float(np.mean(waited)) if waited else None,
            "rounding_of_G_min_max": [float(min(frac)), float(max(frac))] if frac else None,
            "ms_plain_call_median": float(np.median(ms_plain)) if ms_plain else None, "ms_gap_plus_call_median": float(np.median(ms_gap)) if ms_gap else None}
        print("Es/N0 %g dB: %s" % (esn0, json.dumps(result["by_esn0"]["%g" % esn0])), flush=True)
    result["largest_magnitude"] = largest
    result["default_window"] = max(8, -(-2 * largest // 8) * 8)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("largest magnitude %d -> default window %d" % (largest, result["default_window"]))


if __name__ == "__main__":
    main()
