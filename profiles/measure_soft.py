"""What soft-decision decoding costs in the receive chain (TETRA_RX_FLAG_SOFT, include/tetra_rx.h): 4096 channels x 36 000 samples per
call of coded downlinks (8 distinct cells tiled, 25 dB), steady state after warm-up.  One measurement = `--calls` process calls enqueued
back to back between two HIP events (the second behind the last call's tail), as ms per call; reported: the median over `--reps`, for the
two-stream chain and for TETRA_RX_FLAG_ONE_STREAM, plus tetra_rx_stage_ms of the last call.  With the flag the one-stream figure
holds everything the option adds -- the demodulator's symbol write, k_soft, the soft SB1 launch, the soft launch of the other kinds and
the AACH's own launch -- and the stages say where: ms[0] the demodulator launch (symbol write included), ms[2] SB1, ms[3] the other kinds;
what is left of the one-stream difference is k_soft, which no stage event brackets.

    python profiles/measure_soft.py                        # one process: flag off and on -> profiles/r12/soft.json
    python profiles/measure_soft.py --ab PARENT_LIB [--rounds 2]
        three builds -- a build of the parent commit (its libtetra_demod_hip.so), this build with the flag off, this build with the flag
        on -- in fresh processes in alternation; reports each one's medians per round and the parent's own round-to-round spread, which
        is the resolution of the comparison
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "r12", "soft.json")
FLAG_SOFT = 8


def stream(pkg, np, n_channels, n_samples):
    n_slots = n_samples // 510 + 2
    base = []
    for c in range(8):
        bits = pkg.synth.gen_downlink(n_slots, 1200 + c, cell=(300 + c, 2000 + c, c))[0]
        base.append(pkg.synth.gen_channel(n_samples, 1300 + c, bits=bits)[0])
    return np.tile(np.stack(base), (n_channels // 8, 1))


def measure(pkg, torch, d_iq, n_channels, n_samples, flags, calls, warmup, reps):
    R = pkg.rx_binding
    rx = pkg.RxChain(n_channels, n_samples, flags=flags)
    s = torch.cuda.current_stream()
    for _ in range(warmup):
        rx.process_device(d_iq, n_samples, s)
    rx.wait()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(calls):
            rx.process_device(d_iq, n_samples, s)
        rx.rows_device(R.KIND_SCH_F, 0, s)           # the stream waits for the last call's tail
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    blocks = rx.fetch(R.KIND_SCH_F)[0]
    out = {"ms_per_call_median": round(statistics.median(ms), 4), "ms_per_call_min": round(min(ms), 4), "ms_per_call_max": round(max(ms), 4),
           "stage_ms": [round(v, 4) for v in rx.stage_ms()], "schf_rows": int(len(blocks)), "schf_rows_crc_ok": int((blocks["crc_ok"] != 0).sum())}
    rx.close()
    return out


def run(a, flag):
    import numpy as np
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    d_iq = torch.from_numpy(stream(pkg, np, a.channels, a.samples)).cuda()
    fl = FLAG_SOFT if flag else 0
    return {"flag": int(flag), "channels": a.channels, "samples": a.samples, "calls_per_measurement": a.calls, "reps": a.reps,
            "two_stream": measure(pkg, torch, d_iq, a.channels, a.samples, fl, a.calls, a.warmup, a.reps),
            "one_stream": measure(pkg, torch, d_iq, a.channels, a.samples, fl | R.FLAG_ONE_STREAM, a.calls, a.warmup, a.reps)}


def child(lib, flag, a):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(int(flag)), "--calls", str(a.calls), "--warmup", str(a.warmup), "--reps", str(a.reps),
           "--channels", str(a.channels), "--samples", str(a.samples)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(run(a, bool(a.child))), flush=True)
        return
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.ab:
        rounds = []
        for _ in range(a.rounds):          # fresh processes: parent, this build flag off, this build flag on, in alternation
            rounds.append({"parent": child(os.path.abspath(a.ab), False, a), "flag_off": child(None, False, a), "flag_on": child(None, True, a)})
            print(json.dumps(rounds[-1]), flush=True)
        summary = {}
        for mode in ("two_stream", "one_stream"):
            med = {k: [r[k][mode]["ms_per_call_median"] for r in rounds] for k in ("parent", "flag_off", "flag_on")}
            mean = {k: statistics.mean(v) for k, v in med.items()}
            summary[mode] = {"medians_ms": med, "parent_round_to_round_spread_ms": round(max(med["parent"]) - min(med["parent"]), 4),
                             "flag_off_minus_parent_ms": round(mean["flag_off"] - mean["parent"], 4),
                             "flag_on_minus_flag_off_ms": round(mean["flag_on"] - mean["flag_off"], 4)}
        summary["one_stream_stage_ms"] = {k: [r[k]["one_stream"]["stage_ms"] for r in rounds] for k in ("parent", "flag_off", "flag_on")}
        res["three_builds"] = {"rounds": rounds, "summary": summary}
        print(json.dumps(summary), flush=True)
    else:
        res["one_process"] = {"flag_off": run(a, False), "flag_on": run(a, True)}
        print(json.dumps(res["one_process"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
