"""What the extended delivery (include/ext/tetra_rx_out_ext.h) costs, on profiles/measure_rx_out.py's workload: 4096 channels x 36000
samples, two streams, the previous call's blocks of every kind delivered packed into mapped page-locked memory after each call and
waited for one call later.  ONE variant per process (fresh processes are alternated by the caller, parent build and this build through
TETRA_DEMOD_LIB):

  --variant none      process_device only
  --variant classic   + tetra_rx_out_enqueue (packed); runs on the parent build as well
  --variant ext       + tetra_rx_out_enqueue_ext with every row and channel extra, the snapshot armed (this build only)
  --variant armed     classic deliveries with the snapshot armed: the tail's extra kernel alone

--all-flags creates the handle with BITERR | LIST | AACH_RM3014 | SYNC_TOLERANT (needed for ext), else with no flag (the figure of
DESIGN 8.5).  Prints one JSON object: ms per second of signal (best and every round), bytes per delivery."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["none", "classic", "ext", "armed"], required=True)
    ap.add_argument("--all-flags", action="store_true")
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--seconds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    import torch
    import tetra_amd
    from measure_rx_out import workload
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    device = torch.device("cuda", 0)
    C, N = a.channels, a.samples
    d_iq = workload(torch, pkg, device, C, N, a.seconds)
    stream = torch.cuda.current_stream(device)
    flags = R.FLAG_BITERR | R.FLAG_LIST | R.FLAG_AACH_RM3014 | R.FLAG_SYNC_TOLERANT if a.all_flags else 0
    rx = pkg.RxChain(C, N, device=0, flags=flags)
    extras = R.EXT_ROW_ALL | R.EXT_CHAN_ALL if a.variant == "ext" else 0
    if a.variant in ("ext", "armed"):
        rx.set_snapshot(R.EXT_CHAN_ALL if a.all_flags else R.EXT_CHAN_CELL | R.EXT_CHAN_SYNC_STATE)
    bufs = [R.HostBuffer(rx.out_bound(extras=extras)) for _ in range(2)]
    k = 0

    def call():
        nonlocal k
        rx.process_device(d_iq[k % a.seconds], N, stream)
        k += 1

    for _ in range(a.seconds + 2):          # lock loops and synchronisers, fill pools, ramp the clock
        call()
    rx.wait()

    def run():
        pend = None
        rx.wait()
        t0 = time.perf_counter()
        for i in range(a.reps):
            call()
            if a.variant != "none":
                d = rx.deliver(1, packed=True, buf=bufs[i % 2], extras=extras)
                if pend is not None:
                    pend.wait()
                pend = d
        if pend is not None:
            pend.wait()
        rx.wait()
        return (time.perf_counter() - t0) * 1e3 / a.reps, pend

    rounds, d = [], None
    for _ in range(a.rounds):
        ms, d = run()
        rounds.append(round(ms, 3))
    res = {"variant": a.variant, "all_flags": a.all_flags, "lib": os.environ.get("TETRA_DEMOD_LIB", "tree"), "channels": C, "samples_per_channel": N,
           "reps": a.reps, "ms_per_second_two_streams": min(rounds), "rounds_ms": rounds}
    if d is not None:
        res["classic_bytes"] = int(d.header.bytes)
        res["rows_per_kind"] = {int(e.kind): int(e.n_rows) for e in d.header.kinds[:d.header.n_kinds]}
        if d.ext_header is not None:
            res["total_bytes"] = int(d.ext_header.bytes)
    rx.close()
    for b in bufs:
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
