"""The receive chain's one-step hand-off (include/tetra_rx_out.h) against no hand-off and against tetra_rx_fetch, on bench.py's chain
workload: 4096 channels x 36000 samples, 64 coded downlinks (synth.gen_downlink) each used for 64 channels with its own amplitude,
carrier offset and phase, 4 resident seconds streamed round and round.  Two streams (the demodulator of call k+1 beside the tail of
call k).  Variants, alternated in one process:

  none            process_device only
  fetch           + tetra_rx_fetch of every kind of the previous call after each call (pageable numpy, blocking, one kind at a time)
  deliver_packed  + a delivery of every kind of the previous call into mapped page-locked memory, packed bits, waited for one call
                    later (the way a consumer thread would)
  deliver_bytes   the same, one byte per bit

--crc-good: the deliveries keep the CRC-good rows only (count and scan launches before the write).  `delivery_alone_ms`: one delivery
enqueued behind a finished call and waited for, nothing beside it (best of the rounds).

Prints one JSON object: ms per second of signal per variant (best of the rounds), bytes per delivery.  The delivery kernels' own
time comes from a separate run under `rocprofv3 --kernel-trace --stats` (--calls N: just N delivered calls, no timing)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DISTINCT = 64


def workload(torch, pkg, device, C, N, seconds):
    synth = pkg.synth
    n_slots = seconds * N // 510 + 2
    cells = [(200 + c, 3000 + 7 * c, (11 * c + 5) % 64) for c in range(DISTINCT)]
    down = [synth.gen_downlink(n_slots, 7000 + c, cell=cells[c]) for c in range(DISTINCT)]
    nb = synth.needed_bits(seconds * N)
    bits = np.zeros((DISTINCT, nb), np.uint8)
    for c in range(DISTINCT):
        bits[c, : min(nb, down[c][0].size)] = down[c][0][:nb]
    seeds = torch.arange(DISTINCT, dtype=torch.int64, device=device) + 31000
    prm = pkg.synth_gpu.hash_params(torch, device, seeds)
    one = torch.ones(DISTINCT, dtype=torch.float64, device=device)
    base = pkg.synth_gpu.modulate_batch(torch, device, torch.from_numpy(bits).to(device), seconds * N, prm["tau"], 0 * one, one, 0 * one,
                                        esn0_db=25.0, noise_seed=31000)
    g = torch.Generator(device="cpu")
    g.manual_seed(31001)
    amp = torch.empty(C).uniform_(0.05, 1.0, generator=g).to(device).double()
    dw = torch.empty(C).uniform_(-0.05, 0.05, generator=g).to(device).double()
    ph = torch.empty(C).uniform_(-3.14159, 3.14159, generator=g).to(device).double()
    idx = torch.arange(C, device=device) % DISTINCT
    n = torch.arange(seconds * N, device=device, dtype=torch.float64)
    d_iq = [torch.empty((C, N), dtype=torch.complex64, device=device) for _ in range(seconds)]
    for c0 in range(0, C, 256):
        c1 = min(C, c0 + 256)
        rot = torch.polar(amp[c0:c1, None].expand(-1, seconds * N).contiguous(), dw[c0:c1, None] * n[None, :] + ph[c0:c1, None]).to(torch.complex64)
        x = base[idx[c0:c1]] * rot
        for k in range(seconds):
            d_iq[k][c0:c1] = x[:, k * N:(k + 1) * N]
    return d_iq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--seconds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--crc-good", action="store_true", help="deliveries of the CRC-good rows only")
    ap.add_argument("--calls", type=int, default=0, help="profile mode: only N calls with a packed delivery each, no timing")
    a = ap.parse_args()
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    device = torch.device("cuda", 0)
    C, N = a.channels, a.samples
    d_iq = workload(torch, pkg, device, C, N, a.seconds)
    stream = torch.cuda.current_stream(device)
    rx = pkg.RxChain(C, N, device=0)
    bufs = [R.HostBuffer(rx.out_bound()) for _ in range(2)]
    k = 0

    def call():
        nonlocal k
        rx.process_device(d_iq[k % a.seconds], N, stream)
        k += 1

    for _ in range(a.seconds + 2):          # lock loops and synchronisers, fill pools, ramp the clock
        call()
    rx.wait()
    if a.calls:
        for i in range(a.calls):
            call()
            rx.deliver(1, packed=True, crc_good_only=a.crc_good, buf=bufs[i % 2]).wait()
        rx.close()
        print(json.dumps({"profiled_calls": a.calls}))
        return

    def run(variant):
        pend = None
        rx.wait()
        t0 = time.perf_counter()
        for i in range(a.reps):
            call()
            if variant == "fetch":
                for kind in range(R.N_KINDS):
                    rx.fetch(kind, which=1)
            elif variant.startswith("deliver"):
                d = rx.deliver(1, packed=variant == "deliver_packed", crc_good_only=a.crc_good, buf=bufs[i % 2])
                if pend is not None:
                    pend.wait()
                pend = d
        if pend is not None:
            pend.wait()
        rx.wait()
        return (time.perf_counter() - t0) * 1e3 / a.reps, pend

    def alone(packed):
        call()
        rx.wait()
        t0 = time.perf_counter()
        rx.deliver(0, packed=packed, crc_good_only=a.crc_good, buf=bufs[0]).wait()
        return (time.perf_counter() - t0) * 1e3

    variants = ["none", "fetch", "deliver_packed", "deliver_bytes"]
    best = {v: float("inf") for v in variants}
    solo = {"packed": float("inf"), "bytes": float("inf")}
    sizes = {}
    for _ in range(a.rounds):
        for nm in solo:
            solo[nm] = min([solo[nm]] + [alone(nm == "packed") for _ in range(a.reps)])
        for v in variants:
            ms, d = run(v)
            best[v] = min(best[v], ms)
            if d is not None:
                sizes[v] = int(d.header.bytes)
                rows = {int(e.kind): int(e.n_rows) for e in d.header.kinds[:d.header.n_kinds]}
    res = {"channels": C, "samples_per_channel": N, "reps": a.reps, "rounds": a.rounds,
           "crc_good_only": a.crc_good, "ms_per_second_two_streams": {v: round(best[v], 3) for v in variants},
           "delivery_alone_ms": {nm: round(v, 3) for nm, v in solo.items()},
           "delivery_bytes": sizes, "rows_per_kind": rows,
           "fetch_bytes": int(sum(n * (24 + R.type1_bits(kk)) for kk, n in rows.items()))}
    rx.close()
    for b in bufs:
        b.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
