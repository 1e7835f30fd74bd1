"""Times the soft-decision data channels (include/ext/tetra_tch_soft.h) beside their hard siblings and soft SCH/F: 65 536 rows per kind,
HIP events on the launch stream, every shape warmed up, TRIALS windows of REPS launches each -> one JSON line per case with the median,
the fastest and the slowest window.

    rows    TCH/4.8 and TCH/2.4 through tetra_lmac_decode_tch_counted_device (plain 0 / 1 bytes: the packed route) and through
            tetra_lmac_decode_tch_soft_counted_device (int8 values in [-31, 31])
    frames  SCH/F through tetra_lmac_decode_frames_soft_device and TCH/4.8, TCH/2.4 through tetra_lmac_decode_frames_soft_tch_device:
            65 536 NORM_1 frames, 8 per channel 517 bits apart, in rings of 8192 values, the caller's workspace

    python profiles/measure_lmac_tch_soft.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TRIALS, REPS = 65536, 7, 300
FPC, RING = 8, 8192


def timed(torch, s, launch):
    for _ in range(10):
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
    bits = torch.randint(0, 2, (N, 432), dtype=torch.uint8, device=dev, generator=g)
    soft = torch.randint(-31, 32, (N, 432), dtype=torch.int8, device=dev, generator=g)
    si = torch.randint(0, 2 ** 31, (N,), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    ok = torch.zeros(N, dtype=torch.int32, device=dev)
    ring = torch.randint(-31, 32, (N // FPC, RING), dtype=torch.int8, device=dev, generator=g)
    frames = torch.zeros((N, 16), dtype=torch.int32, device=dev)
    ftype = torch.zeros(N, dtype=torch.int32, device=dev)                 # TETRA_TRAIN_NORM_1
    f = torch.arange(N, dtype=torch.int64, device=dev)
    bitnum = (6000 + 131 * (f // FPC) + 517 * (f % FPC)).to(torch.int32)
    listed = torch.arange(N, dtype=torch.int32, device=dev)

    def report(case, kind, n2, t):
        print(json.dumps(dict(case=case, kind=kind, rows=N, trellis_steps=n2 + 4, **t)), flush=True)

    for name, kind, n2 in (("TCH/4.8", lb.T_TCH_4_8, 292), ("TCH/2.4", lb.T_TCH_2_4, 148)):
        ost = (n2 + 7) & ~7
        out = torch.zeros((N, ost), dtype=torch.uint8, device=dev)
        report("rows hard", name, n2, timed(torch, s, lambda: lb.decode_tch_counted_device(kind, bits, N, None, 432, si, None, out, ost, None, s)))
        report("rows soft", name, n2, timed(torch, s, lambda: lb.decode_tch_soft_counted_device(kind, soft, N, None, 432, si, None, out, ost, None, s)))
    for name, kind, n2, entry in (("SCH/F", lb.TPSAP_T_SCH_F, 288, lb.decode_frames_soft), ("TCH/4.8", lb.T_TCH_4_8, 292, lb.decode_frames_soft_tch),
                                  ("TCH/2.4", lb.T_TCH_2_4, 148, lb.decode_frames_soft_tch)):
        ost = (n2 + 7) & ~7
        job = dict(type=kind, blk_num=0, row_frame=listed, n_rows=None, max_rows=N, out_stride=ost, frame_scramb=si,
                   type2=torch.zeros((N, ost), dtype=torch.uint8, device=dev), crc_ok=ok, labels=None)
        ws = torch.zeros(lb.decode_frames_workspace_bytes([job]), dtype=torch.uint8, device=dev)
        report("frames soft", name, n2, timed(torch, s, lambda: entry(frames, ftype, [job], ring, RING, FPC, bitnum, stream=s, d_workspace=ws, counted=False,
                                                                      ranked=False)))


if __name__ == "__main__":
    main()
