"""The wideband receiver (include/tetra_wbrx.h) on a 20 MHz cs16 capture in 0.25 s blocks, 16 coded TETRA downlinks on the bins
BASELINE config 5 uses (bench.py:wideband_config5), three runs:
  (a) the 16 carriers selected      (b) all 800 bins      (c) the 16 carriers, chain on one stream (TETRA_RX_FLAG_ONE_STREAM)
Records ms per block in steady state (blocks enqueued back to back, one synchronisation at the end), the stage times of the last
block, and the CRC-good block counts of a second pass that fetches after every block.  Writes profiles/r08/wbrx.json.

    python profiles/measure_wbrx.py [--blocks 8] [--warmup 2] [--runs abc] [--out profiles/r08/wbrx.json]

For the kernel table run it under `rocprofv3 --kernel-trace --stats -d DIR -o run -- python profiles/measure_wbrx.py --runs a
--blocks 6 --out /dev/null`, then `python profiles/measure_wbrx.py --merge-rocprof DIR/run_results.db` (no GPU) copies the rows of
the front end's and the demodulator's kernels from that database into the JSON."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BINS = (3, 57, 101, 150, 199, 250, 313, 377, 423, 480, 531, 590, 644, 700, 751, 797)
BLOCK = 5000000          # 0.25 s at 20 MHz


def capture(torch, synth, n_blocks):
    """16 coded downlinks (synth.gen_downlink, a cell each) at 36 ksps, band-limited interpolation to 20 MHz, each shifted to its bin's
    centre, over a noise floor; cs16 [n][2] on the GPU."""
    dev = torch.device("cuda")
    L = n_blocks * BLOCK
    N = L * 9 // 5000                            # 36 ksps samples: 20 MHz / 36 kHz = 5000 / 9
    nslots = N // 510 + 2
    x = torch.zeros(L, dtype=torch.complex64, device=dev)
    for i, k in enumerate(BINS):
        bits = synth.gen_downlink(nslots, 900 + i, cell=(200 + i, 3000 + i, i))[0]
        s = torch.from_numpy(synth.gen_channel(N, 1900 + i, bits=bits, amp=1.0)[0].astype(np.complex128)).to(dev)
        S = torch.fft.fft(s)
        Y = torch.zeros(L, dtype=torch.complex128, device=dev)
        Y[: N // 2] = S[: N // 2]
        Y[L - (N - N // 2):] = S[N // 2:]
        kc = k if k < 400 else k - 800
        ph = torch.arange(L, dtype=torch.float64, device=dev) * (2.0 * math.pi * kc / 800)
        x += (torch.fft.ifft(Y) * (L / N) * torch.polar(torch.ones_like(ph), ph)).to(torch.complex64)
        del S, Y, ph, s
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x += 1e-3 * torch.view_as_complex(torch.randn((L, 2), device=dev, generator=g))
    x *= 0.25 / float(x.abs().max())
    return torch.view_as_real(x).mul(32768.0).round().clamp(-32768, 32767).to(torch.int16).contiguous()


def run(pkg, torch, xs, bins, flags, n_blocks, warmup):
    R = pkg.rx_binding
    wb = pkg.WidebandRx(list(bins), max_in=BLOCK, flags=flags)
    blk = [xs[b * BLOCK:(b + 1) * BLOCK] for b in range(n_blocks)]
    for b in range(warmup):
        wb.process_device(blk[b])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in range(warmup, n_blocks):
        wb.process_device(blk[b])
    wb.rx.wait()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / (n_blocks - warmup)
    out = {"n_bins": len(bins), "flags": flags, "ms_per_block": round(ms, 4),
           "front_ms": [round(v, 4) for v in wb.stage_ms()], "chain_stage_ms": [round(v, 4) for v in wb.rx.stage_ms()]}
    # second pass: fetch after every block, count CRC-good blocks on the 16 carriers
    wb.reset()
    good = {k: 0 for k in range(R.N_KINDS)}
    carrier_cols = [j for j, k in enumerate(bins) if k in BINS]
    for b in range(n_blocks):
        wb.process_device(blk[b])
        for k in range(R.N_KINDS):
            blocks, _ = wb.rx.fetch(k)
            ok = blocks[np.isin(blocks["channel"], carrier_cols)]
            good[k] += int((ok["crc_ok"] != 0).sum())
    out["crc_good"] = {name: good[k] for k, name in enumerate(("sb1", "bbk", "sb2", "ndb1", "ndb2", "schf"))}
    cells = wb.rx.cells()
    out["cells_read"] = sum(1 for j in carrier_cols if cells[j].mcc == 200 + BINS.index(bins[j]))
    wb.close()
    return out


def rocprof_rows(db):
    """The front end's and the demodulator's kernels from a rocprofv3 results database (rocpd `top_kernels` view, durations in us)."""
    import sqlite3
    keep = ("resample", "pick_rows", "bin_power", "channelise", "k_fused")
    rows = sqlite3.connect(db).cursor().execute("select name, total_calls, total_duration, average, percentage from top_kernels").fetchall()
    return [{"kernel": n, "calls": int(c), "total_us": round(t, 1), "avg_us": round(a, 2), "percent": round(p, 2)}
            for n, c, t, a, p in rows if any(k in n for k in keep)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", default="abc")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "wbrx.json"))
    ap.add_argument("--merge-rocprof", default=None, metavar="DB")
    a = ap.parse_args()
    if a.merge_rocprof:
        with open(a.out) as f:
            res = json.load(f)
        res["rocprof_kernel_stats"] = {"command": "rocprofv3 --kernel-trace --stats -- python profiles/measure_wbrx.py --runs a --blocks 6",
                                       "kernels": rocprof_rows(a.merge_rocprof)}
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["rocprof_kernel_stats"], indent=1))
        return
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    xs = capture(torch, pkg.synth, a.blocks)
    res = {"capture": "20 MHz cs16, %d blocks of 0.25 s, 16 coded downlinks on config 5's bins" % a.blocks, "warmup_blocks": a.warmup}
    runs = {"a": ("a_16_carriers", BINS, 0), "b": ("b_all_800_bins", tuple(range(800)), 0), "c": ("c_16_carriers_one_stream", BINS, 1)}
    for r in a.runs:
        name, bins, flags = runs[r]
        res[name] = run(pkg, torch, xs, bins, flags, a.blocks, a.warmup)
        print(name, json.dumps(res[name]), flush=True)
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
