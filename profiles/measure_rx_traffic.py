"""What the traffic routing (include/ext/tetra_traffic.h) costs, on profiles/measure_rx_out.py's workload: 4096 channels x 36000 samples
per call.  ONE variant per process (--variant); --job alternates fresh processes of the parent's build (TETRA_DEMOD_LIB, --parent-lib) and
of this build, two rounds of processes, and writes the medians and spreads to --out.

  --variant off    never enabled (runs on the parent's build as well)
  --variant zero   enabled, the table all zero: the routing launches and an empty decode launch
  --variant one    + timeslot 2 of every channel carries TCH/4.8
  --variant two    + timeslot 4 of every channel carries TCH/2.4

--one-stream creates the handle with TETRA_RX_FLAG_ONE_STREAM.  The workload's one-channel bursts carry SCH/F blocks; decoded as TCH they
cost what TCH blocks cost.  Prints one JSON object: ms per call (every round, and their median)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def measure(a):
    import torch
    import tetra_amd
    from measure_rx_out import workload
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    device = torch.device("cuda", 0)
    C, N = a.channels, a.samples
    d_iq = workload(torch, pkg, device, C, N, a.seconds)
    stream = torch.cuda.current_stream(device)
    rx = pkg.RxChain(C, N, device=0, flags=R.FLAG_ONE_STREAM if a.one_stream else 0)
    if a.variant != "off":
        rx.enable_traffic()
        slots = {"zero": {}, "one": {2: R.TCH_4_8}, "two": {2: R.TCH_4_8, 4: R.TCH_2_4}}[a.variant]
        rx.set_traffic([slots] * C, stream=stream)
    k = 0

    def call():
        nonlocal k
        rx.process_device(d_iq[k % a.seconds], N, stream)
        k += 1

    for _ in range(a.seconds + 2):          # lock loops and synchronisers, fill pools, ramp the clock
        call()
    rx.wait()
    rounds = []
    for _ in range(a.rounds):
        rx.wait()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        rx.wait()
        rounds.append(round((time.perf_counter() - t0) * 1e3 / a.reps, 4))
    res = {"variant": a.variant, "one_stream": a.one_stream, "lib": "parent" if os.environ.get("TETRA_DEMOD_LIB") else "tree", "channels": C,
           "samples_per_channel": N, "reps": a.reps, "rounds_ms": rounds, "median_ms": round(statistics.median(rounds), 4)}
    if a.variant != "off":
        res["rows"] = {k: len(rx.fetch_traffic(k)[0]) for k in (R.TCH_7_2, R.TCH_4_8, R.TCH_2_4)}
    res["stage_ms"] = [round(v, 4) for v in rx.stage_ms()]
    rx.close()
    print(json.dumps(res))


def job(a):
    """(build, variant, one stream) in turn, a fresh process each, twice over; the parent's build first and last of every round"""
    plan = [("parent", "off", False), ("tree", "off", False), ("tree", "zero", False), ("tree", "one", False), ("tree", "two", False),
            ("tree", "off", True), ("tree", "two", True), ("parent", "off", True), ("parent", "off", False)]
    runs = []
    for rnd in range(2):
        for lib, variant, one in plan:
            env = dict(os.environ)
            env.pop("TETRA_DEMOD_LIB", None)
            if lib == "parent":
                env["TETRA_DEMOD_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", variant, "--channels", str(a.channels), "--samples", str(a.samples),
                   "--reps", str(a.reps), "--rounds", str(a.rounds)] + (["--one-stream"] if one else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.process_timeout)
            if r.returncode != 0:                     # nothing more is started on the GPU behind a process that failed
                print(r.stdout[-2000:], r.stderr[-4000:])
                return r.returncode or 1
            res = json.loads(r.stdout.strip().splitlines()[-1])
            res["process_round"] = rnd
            runs.append(res)
            print(json.dumps(res), flush=True)
    summary = {}
    for lib, variant, one in sorted(set(plan)):
        ms = [v for r in runs if (r["lib"], r["variant"], r["one_stream"]) == (lib, variant, one) for v in r["rounds_ms"]]
        per = [r["median_ms"] for r in runs if (r["lib"], r["variant"], r["one_stream"]) == (lib, variant, one)]
        summary["%s_%s_%s" % (lib, variant, "one_stream" if one else "two_streams")] = {
            "median_ms": round(statistics.median(ms), 4), "min_ms": min(ms), "max_ms": max(ms), "process_medians_ms": per}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"workload": "%d channels x %d samples per call" % (a.channels, a.samples), "summary": summary, "runs": runs}, f, indent=1)
    print(json.dumps(summary, indent=1))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["off", "zero", "one", "two"])
    ap.add_argument("--one-stream", action="store_true")
    ap.add_argument("--job", action="store_true")
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "rx_traffic.json"))
    ap.add_argument("--process-timeout", type=int, default=150)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--seconds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.job:
        if not a.parent_lib:
            ap.error("--job needs --parent-lib")
        sys.exit(job(a))
    if not a.variant:
        ap.error("--variant or --job")
    measure(a)


if __name__ == "__main__":
    main()
