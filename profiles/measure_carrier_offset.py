"""Per-carrier offsets of the wideband receiver (include/ext/tetra_carrier_offset.h): what they cost and how far they reach.

  python profiles/measure_carrier_offset.py cost --parent-lib PATH [--rounds N] [--out FILE]
      The benchmark's wideband shape (20 MHz cs16, M 800, D 400, its 16-carrier bin list, 0.25 s per call) through WidebandRx in fresh
      processes, in alternation: a build of the parent commit (PATH, loaded through TETRA_DEMOD_LIB), this build with the offsets never
      set, this build with an offset on every slot.  Per process: the resampler stage and the channeliser stage from
      tetra_wbrx_stage_ms (HIP events) and the whole call on the host clock around a device synchronise, medians over the timed calls.
      The parent's own round-to-round spread is what "costs nothing when off" is held against.

  python profiles/measure_carrier_offset.py reach [--out FILE]
      The known-answer band of tests/test_carrier_offset_gpu.py (M 32, D 16, 80 slots; carriers 7 and 20 off their centres by +f and
      -f) with chan_cutoff_rel 2.0 and taps_per_channel 8 and 16, f stepped in 1.5625 kHz units: the largest |f| up to which
      tests/test_wbrx.py's known-answer assertions hold for every carrier at every step below it.

Each prints one JSON line (and writes it to FILE)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BINS16 = (3, 57, 101, 150, 199, 250, 313, 377, 423, 480, 531, 590, 644, 700, 751, 797)
M, D, N_IN = 800, 400, 5000000


def child(mode, warm, calls):
    import torch
    import tetra_amd
    import bench
    pkg = tetra_amd.pkg
    dev = torch.device("cuda", 0)
    x, _ = bench.wideband_tetra(torch, pkg.synth, dev, M, N_IN, {k: 500 + i for i, k in enumerate(BINS16)})
    peak = float(torch.view_as_real(x).abs().max())
    xs = torch.clamp(torch.round(torch.view_as_real(x) * (0.25 * 32768.0 / peak)), -32768, 32767).to(torch.int16).contiguous()
    del x
    wb = pkg.WidebandRx(list(BINS16), max_in=N_IN)
    if mode == "on":      # a few hundred hertz to a few kilohertz, both signs, every slot
        wb.set_offsets(hz=[(-1) ** j * (150.0 + 390.625 * j) for j in range(len(BINS16))])
    s = torch.cuda.current_stream(dev)
    for _ in range(warm):
        wb.process_device(xs, N_IN, s)
    torch.cuda.synchronize()
    whole, chan, res = [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        wb.process_device(xs, N_IN, s)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
        ms = wb.stage_ms()
        chan.append(ms[0])
        res.append(ms[1])
    frames = int(wb.frames_device(0)[1])
    wb.close()
    print(json.dumps({"mode": mode, "resamp_ms": statistics.median(res), "chan_ms": statistics.median(chan), "call_ms": statistics.median(whole),
                      "resamp_ms_min": min(res), "call_ms_min": min(whole), "frames_out": frames}))


def cost(args):
    if not os.path.exists(args.parent_lib):
        raise SystemExit("no parent build at %s" % args.parent_lib)
    runs = {"parent": [], "off": [], "on": []}
    for r in range(args.rounds):
        for mode in ("parent", "off", "on"):
            env = dict(os.environ)
            env.pop("TETRA_DEMOD_LIB", None)
            if mode == "parent":
                env["TETRA_DEMOD_LIB"] = os.path.abspath(args.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--mode", mode, "--warm", str(args.warm), "--calls", str(args.calls)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("child %s failed (%d):\n%s" % (mode, p.returncode, p.stderr[-2000:]))
            runs[mode].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print("round %d %s" % (r, runs[mode][-1]), flush=True)
    res = {"workload": "20 MHz cs16, %d samples per call, M %d, D %d, %d carriers" % (N_IN, M, D, len(BINS16)), "rounds": args.rounds,
           "warm_calls": args.warm, "timed_calls": args.calls, "runs": runs}
    for key in ("resamp_ms", "call_ms", "chan_ms"):
        for mode in runs:
            v = [r[key] for r in runs[mode]]
            res["%s_%s" % (mode, key)] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    for key in ("resamp_ms", "call_ms"):
        p, off, on = (res["%s_%s" % (m, key)] for m in ("parent", "off", "on"))
        res["off_within_parent_spread_" + key] = bool(p["min"] <= off["median"] <= p["max"])
        res["on_minus_parent_" + key] = on["median"] - p["median"]
    frames = N_IN // D
    lines = frames * len(BINS16)                    # every picked element of a row lies in a cache line of its own (a row is 6400 bytes)
    res["resamp_lines_read"] = lines
    res["resamp_on_GBps_at_128B_lines"] = lines * 128.0 / (res["on_resamp_ms"]["median"] * 1e-3) / 1e9
    return res


def reach(args):
    import torch
    import tetra_amd
    from tests.test_carrier_offset_gpu import _capture_offsets
    from tests.test_wbrx import BINS_SMALL, CARRIERS_SMALL, D_SMALL, M_SMALL, _assert_known_answer, _run_collect
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    step_hz = 1562.5
    out = {"band": "M 32, D 16, 80 slots, carriers 7 (+f) and 20 (-f) off centre", "chan_cutoff_rel": 2.0, "step_hz": step_hz, "taps": {}}
    caps = {}
    for P in (8, 16):
        rows, reach_hz, broken = [], 0.0, False
        for i in range(0, 9):
            f = i * step_hz
            if i not in caps:
                caps[i] = _capture_offsets(torch, pkg.synth, M_SMALL, CARRIERS_SMALL, 80, dict(zip(BINS_SMALL, [0.0, f, -f, 0.0])))
            x, cells, tx = caps[i]
            wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=x.shape[0], chan_cutoff_rel=2.0, taps_per_channel=P,
                                offsets_hz=[0.0, f, -f, 0.0])
            got = _run_collect(pkg, wb, x, [0, x.shape[0]])
            try:
                _assert_known_answer(pkg, pkg.synth, got, wb.rx.cells(), cells, tx, 80)
                ok, why = True, ""
            except (AssertionError, ValueError) as e:
                ok, why = False, str(e).split("\n")[0][:120]
            good = [len([r for r in got[R.KIND_SCH_F] if r[0] == c and r[2]]) for c in range(4)]
            wb.close()
            rows.append({"offset_hz": f, "decodes_every_block": ok, "schf_crc_good": good, "why": why})
            print(P, rows[-1], flush=True)
            broken = broken or not ok
            if not broken:
                reach_hz = f
        out["taps"][str(P)] = {"reach_hz": reach_hz, "steps": rows}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cost", "reach", "child"])
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--mode", default="off")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.what == "child":
        child(a.mode, a.warm, a.calls)
    else:
        result = cost(a) if a.what == "cost" else reach(a)
        line = json.dumps(result)
        print(line)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(line + "\n")
