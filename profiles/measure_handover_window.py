"""How far a freshly reset demodulator's bit stream is displaced against a running one's on the same sample timeline: the number the
hand-over's default window (include/ext/tetra_handover.h, TETRA_HANDOVER_DEFAULT_WINDOW) rests on.  CPU only: the oracle demodulator.

Per Es/N0 and seed: the project's synthetic downlink (synth.gen_slot_bits -> synth.gen_channel, random carrier offset, timing, amplitude
and phase), one oracle channel that runs from sample 0 (the donor) and one that starts afresh at a random reset point r (the heir).
The donor has delivered B bits up to r and its frames start at bit numbers = L (mod 510), L its lag against the transmitted bits just
before r; so the hand-over rule expects the heir's frames at (L - B) mod 510 in the heir's numbering, which starts at 0 at r.  The
heir's own lag is measured slot period by slot period over its bits 510 k .. 510 (k + 1), k = 1 .. 6 -- where ASSIST looks first; a
timing slip inside a longer stretch would read as bit errors --, and the figure recorded per stretch is found start - expected start,
folded to (-255, 255].  A stretch (the donor's last 510 bits before r, or one of the heir's) in which more than a tenth of the bits
differ from what was sent at the best lag is not demodulated and says nothing about a lag: counted, not used.

    python profiles/measure_handover_window.py [--seeds 200] [--out profiles/r21/handover_window.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lag_of(rx, tx, guess, span, lo, hi):
    """The d in [-span, span] that minimises the errors of rx[i] == tx[i - guess - d] over i in [lo, hi) -> (d, errors, compared)."""
    best = (None, 1 << 60, 0)
    for d in range(-span, span + 1):
        a, b = max(lo, guess + d), min(hi, rx.size, tx.size + guess + d)
        if b - a < 256:
            continue
        err = int(np.count_nonzero(rx[a:b] != tx[a - guess - d:b - guess - d]))
        if err < best[1]:
            best = (d, err, b - a)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "handover_window.json"))
    args = ap.parse_args()
    import tetra_amd
    synth = tetra_amd.pkg.synth
    from oracle import binding as ob
    n_slots, n_samples = 16, 16 * 510          # 2 samples per symbol, 2 bits per symbol: a sample per bit
    result = {"seeds": args.seeds, "n_samples": n_samples, "heir_slots_compared": [1, 6], "by_esn0": {}}
    for esn0 in (11.0, 20.0, 25.0):
        rows, control = [], []
        for seed in range(args.seeds):
            rng = np.random.default_rng(977 * seed + int(esn0))
            tx = synth.gen_slot_bits(n_slots + 2, 5000 + seed)
            iq, _, prm = synth.gen_channel(n_samples, 100 + seed, esn0_db=esn0, bits=tx)
            r = int(rng.integers(6 * 510, 9 * 510))
            donor, heir = ob.Oracle(), ob.Oracle()
            a = donor.process(iq[:r])["bits"].copy()
            hb = heir.process(iq[r:])["bits"].copy()
            B = a.size
            dl, derr, dn = lag_of(a, tx, 0, 400, B - 510, B)          # donor: a[i] == tx[i - L]
            # heir bit i is the stream's bit B + i if nothing is displaced: heir[i] == tx[i + B - L - d]
            cb = donor.process(iq[r:])["bits"]          # the control: the donor's own continuation is displaced by nothing
            for k in range(1, 7):
                hd, herr, hn = lag_of(hb, tx, dl - B, 255, 510 * k, 510 * (k + 1))
                cd, cerr, cn = lag_of(cb, tx, dl - B, 255, 510 * k, 510 * (k + 1))
                if derr / dn < 0.1 and cerr / cn < 0.1:
                    control.append((cd + 255) % 510 - 255)
                rows.append({"seed": seed, "reset_sample": r, "donor_bits": B, "donor_lag": dl, "donor_ber": derr / dn, "heir_slot": k,
                             "displacement": (hd + 255) % 510 - 255, "heir_ber": herr / hn, "tau": prm["tau"], "cfo": prm["cfo"]})
        disp = np.array([x["displacement"] for x in rows])
        # a lag found on a stream that is mostly errors means nothing: keep those cases apart
        sane = np.array([x["heir_ber"] < 0.1 and x["donor_ber"] < 0.1 for x in rows])
        vals, counts = np.unique(disp[sane], return_counts=True)
        result["by_esn0"]["%g" % esn0] = {
            "donors_not_demodulated": len({x["seed"] for x in rows if x["donor_ber"] >= 0.1}),
            "control_histogram": {str(int(v)): int(c) for v, c in zip(*np.unique(np.array(control, np.int64), return_counts=True))},
            "stretches": len(rows), "stretches_demodulated": int(sane.sum()),
            "histogram": {str(int(v)): int(c) for v, c in zip(vals, counts)},
            "largest_magnitude": int(np.abs(disp[sane]).max()) if sane.any() else None,
            "by_heir_slot": {str(k): {str(int(v)): int(c) for v, c in zip(*np.unique(disp[sane & (np.array([x["heir_slot"] for x in rows]) == k)], return_counts=True))}
                             for k in range(1, 7)}, "rows": rows}
        print("Es/N0 %g dB: %d stretches, %d demodulated, displacement histogram %s" % (esn0, len(rows), int(sane.sum()),
                                                                                  result["by_esn0"]["%g" % esn0]["histogram"]), flush=True)
    largest = max(v["largest_magnitude"] or 0 for v in result["by_esn0"].values())
    result["largest_magnitude"] = largest
    result["default_window"] = min(64, -(-2 * largest // 8) * 8)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for v in result["by_esn0"].values():          # the per-case rows are for the run's log, not for the record
        v.pop("rows")
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("largest magnitude %d -> default window %d" % (largest, result["default_window"]))


if __name__ == "__main__":
    main()
