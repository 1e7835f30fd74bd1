"""What the capture conditioning costs (include/ext/tetra_iqcond.h), on run (a) of profiles/measure_wbrx.py: a 20 MHz cs16 capture in 0.25 s
blocks, 16 coded downlinks on config 5's bins, steady state after warm-up.  One measurement = `--blocks` blocks enqueued back to back on one
stream between two HIP events (the second behind the last block's tail), as ms per block; reported: the median over `--reps`.

    python profiles/measure_iqcond.py                                          # map unset / set: ms per block, k_channelise_fft per launch
        (HIP events around the kernel, tetra_chan_last_kernel_ms, 12 500 frames) for cs16 and complex64, and tetra_iq_stats_device on
        5 M cs16 samples -> profiles/r11/iqcond.json
    python profiles/measure_iqcond.py --ab PARENT_LIB [--rounds 2]             # map never set: this build against a build of the parent
        commit (its libtetra_demod_hip.so), fresh processes in alternation; reports each build's median per round and the round-to-round
        spread of the parent's own median, which is the resolution of the comparison
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_wbrx import BINS, BLOCK, capture  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r11", "iqcond.json")
MAP = (1.0, 0.0, -0.0524, 0.9537, 0.011, -0.007)          # what the solver gives for g = 1.05, phi = 3 degrees and a DC offset


def per_block(pkg, torch, xs, with_map, n_blocks, warmup, reps):
    R = pkg.rx_binding
    wb = pkg.WidebandRx(list(BINS), max_in=BLOCK)
    if with_map:
        wb.set_input_map(MAP)
    blk = [xs[b * BLOCK:(b + 1) * BLOCK] for b in range(xs.shape[0] // BLOCK)]
    s = torch.cuda.current_stream()
    step = [0]

    def block():
        wb.process_device(blk[step[0] % len(blk)], BLOCK, s)
        step[0] += 1

    for _ in range(warmup):
        block()
    wb.rx.wait()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(n_blocks):
            block()
        wb.rx.rows_device(R.KIND_SB1, 0, s)          # the stream waits for the last block's tail
        e1.record(s)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / n_blocks)
    out = {"map": bool(with_map), "blocks_per_measurement": n_blocks, "reps": reps, "ms_per_block_median": round(statistics.median(ms), 4),
           "ms_per_block_min": round(min(ms), 4), "ms_per_block_max": round(max(ms), 4), "front_ms": [round(v, 4) for v in wb.stage_ms()]}
    wb.close()
    return out


def kernel_us(pkg, torch, x, with_map, warmup=30, reps=40):
    """k_channelise_fft on 12 500 frames (5 M samples), HIP events around the kernel: median us per launch."""
    ch = pkg.Channeliser(800, 8, 400, max_in=BLOCK)
    if with_map:
        ch.set_input_map(MAP)
    out = torch.zeros((BLOCK // 400, 800), dtype=torch.complex64, device="cuda")
    us = []
    for i in range(warmup + reps):
        ch.process_device(x, BLOCK, out)
        torch.cuda.synchronize()
        if i >= warmup:
            us.append(1e3 * ch.last_kernel_ms())
    ch.close()
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def stats_us(pkg, torch, xs, warmup=10, reps=40):
    """tetra_iq_stats_device on 5 M cs16 samples: the whole call as the host sees it (scratch allocation, two launches, the 40-byte copy
    back and the wait), median us."""
    x = xs[:BLOCK]
    us = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pkg.iq_stats(x)
        if i >= warmup:
            us.append(1e6 * (time.perf_counter() - t0))
    med = statistics.median(us)
    return {"samples": BLOCK, "bytes_read": 4 * BLOCK, "call_median_us": round(med, 1), "call_min_us": round(min(us), 1),
            "GB_per_s_at_the_median": round(4 * BLOCK / med / 1e3, 1)}


def child(lib, args):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--unset-only", "--blocks", str(args.blocks), "--warmup", str(args.warmup),
           "--reps", str(args.reps), "--capture-blocks", str(args.capture_blocks), "--out", "/dev/null"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])["map_unset"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--capture-blocks", type=int, default=4)
    ap.add_argument("--unset-only", action="store_true", help="ms per block with no map set, nothing else (what --ab runs in each process)")
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = {}
    if a.out != "/dev/null" and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.ab:
        rounds = []
        for _ in range(a.rounds):          # fresh processes, parent and this build in alternation
            rounds.append({"parent": child(os.path.abspath(a.ab), a), "this": child(None, a)})
        pm = [r["parent"]["ms_per_block_median"] for r in rounds]
        tm = [r["this"]["ms_per_block_median"] for r in rounds]
        res["map_never_set_vs_parent"] = {"rounds": rounds, "parent_medians_ms": pm, "this_medians_ms": tm,
                                          "parent_round_to_round_spread_ms": round(max(pm) - min(pm), 4),
                                          "this_minus_parent_ms": round(statistics.mean(tm) - statistics.mean(pm), 4)}
        print(json.dumps(res["map_never_set_vs_parent"]), flush=True)
    else:
        import torch
        import tetra_amd
        pkg = tetra_amd.pkg
        xs = capture(torch, pkg.synth, a.capture_blocks)
        res["capture"] = "20 MHz cs16, %d blocks of 0.25 s cycled, 16 coded downlinks on config 5's bins, 16 slots" % a.capture_blocks
        res["map_unset"] = per_block(pkg, torch, xs, False, a.blocks, a.warmup, a.reps)
        if not a.unset_only:
            res["map_set"] = per_block(pkg, torch, xs, True, a.blocks, a.warmup, a.reps)
            x16 = xs[:BLOCK]
            x64 = torch.view_as_complex((x16.to(torch.float32) / 32768.0).contiguous())
            res["k_channelise_fft_us"] = {"cs16": {"map_unset": kernel_us(pkg, torch, x16, False), "map_set": kernel_us(pkg, torch, x16, True)},
                                          "complex64": {"map_unset": kernel_us(pkg, torch, x64, False), "map_set": kernel_us(pkg, torch, x64, True)}}
            res["iq_stats_device"] = stats_us(pkg, torch, xs)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
