"""Times the coded data channels interleaved over N blocks (include/ext/tetra_tch_nblk.h) beside their N = 1 siblings: 65 536 output blocks
per case, HIP events on the launch stream, every shape warmed up, TRIALS windows of REPS launches each -> one JSON line per case with the
median, the fastest and the slowest window, and the ratio of the median to the sibling's.

    sibling   tetra_lmac_decode_tch_counted_device (plain 0 / 1 bytes: the packed route) / tetra_lmac_decode_tch_soft_counted_device on
              65 536 rows
    N = 1, 4, 8   tetra_lmac_decode_tch_nblk_device / _soft_device: 1024 streams of 64 + N - 1 received rows laid end to end in the pool,
              every stream's 64 sliding windows (lmac_binding.tch_windows), so a workgroup is one stream

    python profiles/measure_lmac_tch_nblk.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS, PER_STREAM, TRIALS, REPS = 65536, 64, 9, 300


def timed(torch, s, launch):
    for _ in range(20):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(TRIALS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(REPS):
            launch()
        e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / REPS)
    return {"us_median": round(1e3 * statistics.median(ms), 2), "us_min": round(1e3 * min(ms), 2), "us_max": round(1e3 * max(ms), 2)}


def main():
    import torch
    sys.path.insert(0, ROOT)
    import tetra_amd
    lb = tetra_amd.pkg.lmac_binding
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    s = torch.cuda.current_stream(dev)
    streams = BLOCKS // PER_STREAM
    rows_max = streams * (PER_STREAM + 7)
    bits = torch.randint(0, 2, (rows_max, 432), dtype=torch.uint8, device=dev, generator=g)
    soft = torch.randint(-31, 32, (rows_max, 432), dtype=torch.int8, device=dev, generator=g)
    si = torch.randint(0, 2 ** 31, (rows_max,), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    for name, kind, n2 in (("TCH/4.8", lb.T_TCH_4_8, 292), ("TCH/2.4", lb.T_TCH_2_4, 148)):
        ost = (n2 + 7) & ~7
        out = torch.zeros((BLOCKS, ost), dtype=torch.uint8, device=dev)
        for mode, pool, sibling, entry in (("hard", bits, lb.decode_tch_counted_device, lb.decode_tch_nblk_device),
                                           ("soft", soft, lb.decode_tch_soft_counted_device, lb.decode_tch_nblk_soft_device)):
            base = timed(torch, s, lambda: sibling(kind, pool, BLOCKS, None, 432, si, None, out, ost, None, s))
            print(json.dumps(dict(case="sibling", mode=mode, kind=name, blocks=BLOCKS, **base)), flush=True)
            for n in (1, 4, 8):
                n_rows = streams * (PER_STREAM + n - 1)
                win = torch.from_numpy(lb.tch_windows([PER_STREAM + n - 1] * streams, n)).to(dev)
                assert win.shape == (BLOCKS, n) and int(win.max()) == n_rows - 1
                t = timed(torch, s, lambda: entry(kind, n, pool, n_rows, 432, si, None, win, BLOCKS, None, out, ost, None, s))
                print(json.dumps(dict(case="nblk", mode=mode, kind=name, n=n, blocks=BLOCKS, pool_rows=n_rows, **t,
                                      ratio_to_sibling=round(t["us_median"] / base["us_median"], 2))), flush=True)


if __name__ == "__main__":
    main()
