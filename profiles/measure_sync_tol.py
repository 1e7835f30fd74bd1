"""What the burst synchroniser's tolerant lock costs in the receive chain (TETRA_RX_FLAG_SYNC_TOLERANT, include/ext/tetra_sync_tol.h): the
stream and the measurement of profiles/measure_soft.py -- 4096 channels x 36 000 samples per call of coded downlinks at 25 dB, steady
state, ms per call on two streams and on one, tetra_rx_stage_ms of the last call -- with the flag off and on.  The synchroniser is
ms[1]; the extra frames it delivers show in the decode stages ms[2] (SB1) and ms[3] (the other kinds).

    python profiles/measure_sync_tol.py                       # one process, this build: flag off / on
    python profiles/measure_sync_tol.py --ab PARENT_LIB [--rounds 2]
        fresh processes in alternation -- a build of the parent commit and this build with the flag off, then both with the flag on (the
        parent's only where it has the tolerant lock) -- with each one's medians per round, the parent's own round-to-round spread (the
        resolution of the comparison), the stages and the rows delivered
    python profiles/measure_sync_tol.py --ab PARENT_LIB --swap
        the same with this build (flag off) in front of the parent build in every round, recorded beside the first as builds_swapped:
        a difference that follows the build and not the position in the round is the build's
Writes profiles/r15/sync_tol.json (--out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import measure_soft  # noqa: E402  (the stream and the timing loop)

OUT = os.path.join(ROOT, "profiles", "r15", "sync_tol.json")
FLAG_SYNC_TOLERANT = 128


def run(a, tolerant):
    import numpy as np
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    d_iq = torch.from_numpy(measure_soft.stream(pkg, np, a.channels, a.samples)).cuda()
    fl = FLAG_SYNC_TOLERANT if tolerant else 0
    out = {"tolerant": int(tolerant), "channels": a.channels, "samples": a.samples, "calls_per_measurement": a.calls, "reps": a.reps,
           "two_stream": measure_soft.measure(pkg, torch, d_iq, a.channels, a.samples, fl, a.calls, a.warmup, a.reps),
           "one_stream": measure_soft.measure(pkg, torch, d_iq, a.channels, a.samples, fl | R.FLAG_ONE_STREAM, a.calls, a.warmup, a.reps)}
    # the rows of a steady-state call (the second call of a fresh handle: the first one acquires)
    rx = pkg.RxChain(a.channels, a.samples, flags=fl)
    for _ in range(2):
        rx.process_device(d_iq, a.samples, torch.cuda.current_stream())
    rx.wait()
    out["rows_per_kind"] = [rx.count(k) for k in range(R.N_KINDS)]
    rx.close()
    return out


def child(lib, tolerant, a):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(int(tolerant)), "--calls", str(a.calls), "--warmup", str(a.warmup),
           "--reps", str(a.reps), "--channels", str(a.channels), "--samples", str(a.samples)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


CONFIGS = (("parent", True, 0), ("off", False, 0), ("parent_on", True, 1), ("on", False, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--swap", action="store_true", help="this build with the flag off runs first in every round, the parent build second: tells a "
                    "difference between the builds from an effect of the position in the round; recorded under builds_swapped")
    ap.add_argument("--parent-on", action="store_true", help="the parent build has the tolerant lock too: measure it with the flag on beside this build's")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(run(a, a.child == "1")), flush=True)
        return
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.ab:
        rounds = []
        for _ in range(a.rounds):
            order = (CONFIGS[1], CONFIGS[0], CONFIGS[3], CONFIGS[2]) if a.swap else CONFIGS
            order = [c for c in order if a.parent_on or c[0] != "parent_on"]
            rounds.append({name: child(os.path.abspath(a.ab) if parent else None, tolerant, a) for name, parent, tolerant in order})
            print(json.dumps(rounds[-1]), flush=True)
        names = [c[0] for c in CONFIGS if a.parent_on or c[0] != "parent_on"]
        s = {}
        for mode in ("two_stream", "one_stream"):
            med = {n: [r[n][mode]["ms_per_call_median"] for r in rounds] for n in names}
            mean = {n: statistics.mean(v) for n, v in med.items()}
            spread = max(med["parent"]) - min(med["parent"])
            s[mode] = {"medians_ms": med, "parent_round_to_round_spread_ms": round(spread, 4),
                       "flag_off_minus_parent_ms": round(mean["off"] - mean["parent"], 4),
                       "flag_off_inside_parent_spread": bool(min(med["parent"]) <= mean["off"] <= max(med["parent"])),
                       "flag_off_not_above_parent_spread": bool(mean["off"] <= max(med["parent"])),
                       "flag_on_minus_flag_off_ms": round(mean["on"] - mean["off"], 4)}
            if a.parent_on:                 # every median of this build against the parent's range, rule by rule
                s[mode].update({"parent_on_round_to_round_spread_ms": round(max(med["parent_on"]) - min(med["parent_on"]), 4),
                                "flag_on_minus_parent_on_ms": round(mean["on"] - mean["parent_on"], 4),
                                "every_flag_off_median_not_above_parent_range": bool(max(med["off"]) <= max(med["parent"])),
                                "every_flag_on_median_not_above_parent_on_range": bool(max(med["on"]) <= max(med["parent_on"]))})
        s["one_stream_stage_ms"] = {n: [r[n]["one_stream"]["stage_ms"] for r in rounds] for n in names}
        s["synchroniser_stage_ms_per_round"] = {n: [r[n]["one_stream"]["stage_ms"][1] for r in rounds] for n in names}
        s["synchroniser_stage_ms"] = {n: round(statistics.mean(r[n]["one_stream"]["stage_ms"][1] for r in rounds), 4) for n in names}
        s["decode_stages_ms"] = {n: round(statistics.mean(r[n]["one_stream"]["stage_ms"][2] + r[n]["one_stream"]["stage_ms"][3] for r in rounds), 4) for n in names}
        s["rows_per_kind"] = {n: rounds[-1][n]["rows_per_kind"] for n in names}
        res["builds_swapped" if a.swap else "builds"] = {"rounds": rounds, "summary": s}
        print(json.dumps(s), flush=True)
    else:
        res["one_process"] = {"on" if t else "off": run(a, t) for t in (0, 1)}
        print(json.dumps(res["one_process"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
