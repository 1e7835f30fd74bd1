"""What retuning costs (include/tetra_retune.h), on run (a) of profiles/measure_wbrx.py: a 20 MHz cs16 capture in 0.25 s blocks, 16 coded
downlinks on config 5's bins, 16 slots, steady state after warm-up.  One measurement = `--blocks` blocks enqueued back to back on one
stream between two HIP events (the second behind the last block's tail), as ms per block; reported: the median over `--reps`.

  --mode none   no retune ever (what every caller pays for the history ring: one k_keep_rows launch per block)
  --mode one    one slot moved before every block (slot i mod 16: off its carrier to a free bin, back 16 blocks later)
  --mode all    all 16 slots moved before every block (the bin list rotated by one)

    python profiles/measure_retune.py --mode none one all                      # one process, the three modes, -> profiles/r10/retune.json
    python profiles/measure_retune.py --ab PARENT_LIB [--rounds 2]             # mode none: this build against a build of the parent
        commit (its libtetra_demod_hip.so), fresh processes in alternation; reports each build's median per round and the
        round-to-round spread of the parent's own median, which is the resolution of the comparison
    rocprofv3 --kernel-trace --stats --output-format rocpd csv -d DIR -o run -- python profiles/measure_retune.py --mode all --reps 2 --out /dev/null
    python profiles/measure_retune.py --merge-rocprof DIR/run_results.db --merge-trace DIR/run_kernel_trace.csv
        (no GPU) the retune's own launches, and the trace's evidence of the two-stream overlap, into the JSON
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from measure_wbrx import BINS, BLOCK, capture  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "r10", "retune.json")


def measure(pkg, torch, xs, mode, n_blocks, warmup, reps):
    R = pkg.rx_binding
    bins = list(BINS)
    wb = pkg.WidebandRx(bins, max_in=BLOCK)
    blk = [xs[b * BLOCK:(b + 1) * BLOCK] for b in range(xs.shape[0] // BLOCK)]
    s = torch.cuda.current_stream()
    step = [0]

    def block():
        i = step[0]
        step[0] += 1
        if mode == "one":          # slot i mod 16 leaves its carrier for a free bin 20 further on, and comes back 16 blocks later
            j = i % 16
            bins[j] = (BINS[j] + 20) % 800 if bins[j] == BINS[j] else BINS[j]
            wb.retune(bins, s)
        elif mode == "all":
            bins.append(bins.pop(0))
            wb.retune(bins, s)
        wb.process_device(blk[i % len(blk)], BLOCK, s)

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
    out = {"mode": mode, "blocks_per_measurement": n_blocks, "reps": reps, "ms_per_block_median": round(statistics.median(ms), 4),
           "ms_per_block_min": round(min(ms), 4), "ms_per_block_max": round(max(ms), 4),
           "front_ms": [round(v, 4) for v in wb.stage_ms()], "chain_stage_ms": [round(v, 4) for v in wb.rx.stage_ms()]}
    if mode != "none":
        out["retunes"], out["slots_moved"] = wb.retune_count()
    wb.close()
    return out


def rocprof_rows(db):
    """The retune's own launches and the per-block kernels next to them (rocpd `top_kernels` view, durations in us)."""
    import sqlite3
    keep = ("k_keep_rows", "k_retune_columns", "k_reset_demod", "k_restart_tail", "resample", "pick_rows", "channelise", "k_fused", "k_burst_sync")
    cur = sqlite3.connect(db).cursor()
    rows = cur.execute("select name, total_calls, total_duration, average, percentage from top_kernels").fetchall()
    return [{"kernel": n, "calls": int(c), "total_us": round(t, 1), "avg_us": round(a, 2), "percent": round(p, 2)}
            for n, c, t, a, p in rows if any(k in n for k in keep)]


def trace_overlap(csv_path):
    """From rocprofv3's kernel trace (CSV): how many k_fused launches ran while a kernel of the previous block's tail ran on another
    queue (the demodulator of block k + 1 beside the tail of block k), and the idle time between a k_reset_demod and the k_fused
    behind it on the same queue (it holds the next call's own front-end kernels; a host round trip would show on top of them)."""
    import csv
    with open(csv_path) as f:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"]) for r in csv.DictReader(f)]
    rows.sort(key=lambda r: r[1])
    fused = [r for r in rows if "k_fused" in r[0]]
    beside, gaps = 0, []
    for f in fused:
        if any(r[3] != f[3] and r[1] < f[2] and r[2] > f[1] for r in rows):
            beside += 1
        prev = [r for r in rows if r[3] == f[3] and r[2] <= f[1] and "k_reset_demod" in r[0]]
        if prev and not any("k_fused" in r[0] and prev[-1][2] <= r[1] < f[1] for r in rows):
            gaps.append((f[1] - prev[-1][2]) / 1e3)
    return {"fused_launches": len(fused), "fused_launches_beside_a_kernel_on_another_queue": beside,
            "reset_demod_end_to_next_fused_start_us_median": round(statistics.median(gaps), 2) if gaps else None,
            "reset_demod_end_to_next_fused_start_us_max": round(max(gaps), 2) if gaps else None}


def child(lib, args):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--mode", "none", "--blocks", str(args.blocks), "--warmup", str(args.warmup),
           "--reps", str(args.reps), "--capture-blocks", str(args.capture_blocks), "--out", "/dev/null"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])["none"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", nargs="+", default=["none", "one", "all"], choices=["none", "one", "all"])
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--capture-blocks", type=int, default=4)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--merge-rocprof", default=None, metavar="DB")
    ap.add_argument("--merge-trace", default=None, metavar="CSV")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = {}
    if a.out != "/dev/null" and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.merge_rocprof:
        res["rocprof_kernel_stats"] = {"command": "rocprofv3 --kernel-trace --stats -- python profiles/measure_retune.py --mode all --reps 2",
                                       "kernels": rocprof_rows(a.merge_rocprof)}
        if a.merge_trace:
            res["rocprof_kernel_stats"]["two_stream_overlap"] = trace_overlap(a.merge_trace)
    elif a.ab:
        rounds = []
        for _ in range(a.rounds):          # fresh processes, parent and this build in alternation
            rounds.append({"parent": child(os.path.abspath(a.ab), a), "this": child(None, a)})
        pm = [r["parent"]["ms_per_block_median"] for r in rounds]
        tm = [r["this"]["ms_per_block_median"] for r in rounds]
        res["no_retune_vs_parent"] = {"rounds": rounds, "parent_medians_ms": pm, "this_medians_ms": tm,
                                      "parent_round_to_round_spread_ms": round(max(pm) - min(pm), 4),
                                      "this_minus_parent_ms": round(statistics.mean(tm) - statistics.mean(pm), 4)}
        print(json.dumps(res["no_retune_vs_parent"]), flush=True)
    else:
        import torch
        import tetra_amd
        pkg = tetra_amd.pkg
        xs = capture(torch, pkg.synth, a.capture_blocks)
        res["capture"] = "20 MHz cs16, %d blocks of 0.25 s cycled, 16 coded downlinks on config 5's bins, 16 slots" % a.capture_blocks
        for m in a.mode:
            res[m] = measure(pkg, torch, xs, m, a.blocks, a.warmup, a.reps)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
