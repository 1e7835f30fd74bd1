"""What the channel bit-error counts cost in the receive chain (TETRA_RX_FLAG_BITERR, include/ext/tetra_biterr.h): the stream and the
measurement of profiles/measure_soft.py -- 4096 channels x 36 000 samples per call of coded downlinks, steady state, ms per call on two
streams and on one, tetra_rx_stage_ms of the last call -- for the hard route and for TETRA_RX_FLAG_SOFT, each with the flag off and on.
The counts live in the decode launches, so they show in ms[2] (SB1) and ms[3] (the other kinds' decode, which with the flag also holds
the link kernel behind it).

    python profiles/measure_biterr.py                       # one process, this build: hard / soft x flag off / on
    python profiles/measure_biterr.py --ab PARENT_LIB [--rounds 2]
        fresh processes in alternation -- a build of the parent commit (hard, soft), this build with the flag off (hard, soft) and on
        (hard, soft) -- with each one's medians per round, the parent's own round-to-round spread (the resolution of the comparison)
        and the decode stages' growth
Writes profiles/r14/biterr.json (--out).
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

OUT = os.path.join(ROOT, "profiles", "r14", "biterr.json")
FLAG_SOFT, FLAG_BITERR = 8, 32


def run(a, soft, count):
    import numpy as np
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    d_iq = torch.from_numpy(measure_soft.stream(pkg, np, a.channels, a.samples)).cuda()
    fl = (FLAG_SOFT if soft else 0) | (FLAG_BITERR if count else 0)
    out = {"soft": int(soft), "biterr": int(count), "channels": a.channels, "samples": a.samples, "calls_per_measurement": a.calls, "reps": a.reps,
           "two_stream": measure_soft.measure(pkg, torch, d_iq, a.channels, a.samples, fl, a.calls, a.warmup, a.reps),
           "one_stream": measure_soft.measure(pkg, torch, d_iq, a.channels, a.samples, fl | R.FLAG_ONE_STREAM, a.calls, a.warmup, a.reps)}
    if count:      # what the figures say on this stream
        rx = pkg.RxChain(a.channels, a.samples, flags=fl)
        rx.process_device(d_iq, a.samples, torch.cuda.current_stream())
        links = rx.links(0, 8)
        rx.close()
        out["links_first_8_channels"] = links
    return out


def child(lib, soft, count, a):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "%d%d" % (soft, count), "--calls", str(a.calls), "--warmup", str(a.warmup),
           "--reps", str(a.reps), "--channels", str(a.channels), "--samples", str(a.samples)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


CONFIGS = (("parent_hard", True, 0, 0), ("parent_soft", True, 1, 0), ("off_hard", False, 0, 0), ("off_soft", False, 1, 0),
           ("on_hard", False, 0, 1), ("on_soft", False, 1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(run(a, a.child[0] == "1", a.child[1] == "1")), flush=True)
        return
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.ab:
        rounds = []
        for _ in range(a.rounds):
            rounds.append({name: child(os.path.abspath(a.ab) if parent else None, soft, count, a) for name, parent, soft, count in CONFIGS})
            print(json.dumps(rounds[-1]), flush=True)
        summary = {}
        for route in ("hard", "soft"):
            names = ["%s_%s" % (p, route) for p in ("parent", "off", "on")]
            s = {}
            for mode in ("two_stream", "one_stream"):
                med = {n: [r[n][mode]["ms_per_call_median"] for r in rounds] for n in names}
                mean = {n: statistics.mean(v) for n, v in med.items()}
                s[mode] = {"medians_ms": med, "parent_round_to_round_spread_ms": round(max(med[names[0]]) - min(med[names[0]]), 4),
                           "flag_off_minus_parent_ms": round(mean[names[1]] - mean[names[0]], 4),
                           "flag_on_minus_flag_off_ms": round(mean[names[2]] - mean[names[1]], 4)}
            s["one_stream_stage_ms"] = {n: [r[n]["one_stream"]["stage_ms"] for r in rounds] for n in names}
            decode = {n: statistics.mean(r[n]["one_stream"]["stage_ms"][2] + r[n]["one_stream"]["stage_ms"][3] for r in rounds) for n in names}
            s["decode_stages_ms"] = {n: round(v, 4) for n, v in decode.items()}
            s["flag_on_share_of_decode_stages"] = round((decode[names[2]] - decode[names[1]]) / decode[names[1]], 4)
            s["two_stream_not_above_one_stream_with_flag"] = statistics.mean(s["two_stream"]["medians_ms"][names[2]]) <= statistics.mean(s["one_stream"]["medians_ms"][names[2]])
            summary[route] = s
        res["builds"] = {"rounds": rounds, "summary": summary}
        print(json.dumps(summary), flush=True)
    else:
        res["one_process"] = {"%s_%s" % ("on" if count else "off", "soft" if soft else "hard"): run(a, soft, count) for soft in (0, 1) for count in (0, 1)}
        print(json.dumps(res["one_process"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
