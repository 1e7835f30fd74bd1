"""What the CRC-aided list decoding (TETRA_RX_FLAG_LIST, include/ext/tetra_list.h) gains and what it costs.

    python profiles/measure_list.py --benefit
        CPU only.  One second (36 000 samples) of five coded downlinks at Es/N0 = 11 dB through the oracle demodulator and the
        reference-free pipeline of tests/list_pipeline.py (the numpy definition), hard decisions and soft values, T = 1, 2, 4, 8:
        CRC-good blocks per kind without and with the option, the rank histogram, and false accepts -- rescued rows whose type-1 bits
        are not among the payloads the transmitter sent.
    python profiles/measure_list.py [--ab PARENT_LIB] [--rounds 2]
        GPU.  The chain at 4096 channels x 36 000 samples per call, ms per call on two streams and on one (the timing loop of
        profiles/measure_soft.py), on a clean input (25 dB: no row fails) and on an 11 dB input, with the flag off and on; --ab adds a
        build of the parent commit in fresh processes in alternation, with the parent's own round-to-round spread as the resolution
        of the comparison.  With the flag the record holds the failed and rescued rows of one call.
Writes profiles/r16/list_benefit.json / profiles/r16/list_cost.json (--out).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

OUT_DIR = os.path.join(ROOT, "profiles", "r16")
FLAG_LIST = 512
KIND_NAMES = {0: "sb1", 2: "sb2", 3: "ndb1", 4: "ndb2", 5: "schf"}


def benefit(a):
    import numpy as np
    import tetra_amd
    from oracle import binding as oracle
    from tests import list_pipeline as LP
    from tests import soft_pipeline as sp
    synth = tetra_amd.pkg.synth
    oracle.build()
    n_slots = a.samples // 510 + 2
    res = {"esn0_db": a.esn0, "channels": 5, "samples": a.samples, "routes": {}}
    streams = []
    for c in range(5):
        bits, sent = synth.gen_downlink(n_slots, 9000 + c, cell=(300 + c, 2000 + c, 1 + c))
        iq = synth.gen_channel(a.samples, 9100 + c, bits=bits, esn0_db=a.esn0)[0].astype(np.complex64)
        b, nb, sym, _ = oracle.process_batch(iq[None, :], want_sym=True)
        streams.append((b[0][:nb[0]], sp.quantise_np(sym[0][:nb[0] // 2]), {k: {bytes(p.tobytes()) for _, p in v} for k, v in sent.items()}))
    for route in ("hard", "soft"):
        per_T = {}
        for T in (0, 1, 2, 4, 8):
            good = {n: 0 for n in KIND_NAMES.values()}
            total = dict(good)
            hist = [0] * 9
            false_accepts = false_ml = 0
            for c, (bits, soft, sent) in enumerate(streams):
                rows = LP.channel_rows(oracle, bits, c, T, soft if route == "soft" else None)
                for (k, _, _), v in rows.items():
                    name = KIND_NAMES[k]
                    total[name] += 1
                    good[name] += v[0]
                    if v[4] > 0:
                        hist[v[4]] += 1
                        false_accepts += v[3] not in sent[name]
                    elif v[0]:
                        false_ml += v[3] not in sent[name]
            per_T[str(T)] = {"crc_good": good, "blocks": total, "rank_histogram_1_to_8": hist[1:], "rescued": sum(hist),
                             "false_accepts_among_rescued": int(false_accepts), "wrong_payloads_among_ml_good": int(false_ml)}
            print(route, "T", T, json.dumps(per_T[str(T)]), flush=True)
        for T in (1, 2, 4, 8):
            assert all(per_T[str(T)]["crc_good"][n] >= per_T["0"]["crc_good"][n] for n in KIND_NAMES.values())
        res["routes"][route] = per_T
    return res


# eight downlinks on which, at 11 dB and 36 000 samples, the reference-free pipeline (tests/list_pipeline.py) has 6 to 13 failed coded
# rows each and rescues 2 or 3 of them with four candidates: a cost input on which the rescue really runs
SEEDS = (71, 70, 4, 30, 60, 43, 27, 11)


def stream(pkg, np, n_channels, n_samples, esn0):
    n_slots = n_samples // 510 + 2
    base = []
    for seed in SEEDS:
        bits = pkg.synth.gen_downlink(n_slots, 8100 + seed, cell=(200 + seed % 50, 3000 + seed, 9 + seed % 40))[0]
        base.append(pkg.synth.gen_channel(n_samples, 8200 + seed, bits=bits, esn0_db=esn0)[0])
    return np.tile(np.stack(base), (n_channels // 8, 1))


def run(a, noisy, on):
    import numpy as np
    import torch
    import tetra_amd
    import measure_soft
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    d_iq = torch.from_numpy(stream(pkg, np, a.channels, a.samples, a.esn0 if noisy else 25.0).astype(np.complex64)).cuda()
    fl = FLAG_LIST if on else 0
    out = {"input": "%g dB" % (a.esn0 if noisy else 25.0), "list": int(on), "channels": a.channels, "samples": a.samples,
           "two_stream": measure_soft.measure(pkg, torch, d_iq, a.channels, a.samples, fl, a.calls, a.warmup, a.reps),
           "one_stream": measure_soft.measure(pkg, torch, d_iq, a.channels, a.samples, fl | R.FLAG_ONE_STREAM, a.calls, a.warmup, a.reps)}
    if on:      # the rows of the first two calls of a fresh handle (the timed calls repeat the second)
        rx = pkg.RxChain(a.channels, a.samples, flags=fl)
        s = torch.cuda.current_stream()
        per_call = []
        for _ in range(2):
            rx.process_device(d_iq, a.samples, s)
            ranks = np.concatenate([rx.fetch_list_rank(k) for k in KIND_NAMES])
            per_call.append((int(ranks.size), int((ranks != 0).sum()), int((ranks > 0).sum())))
        rx.close()
        out["rows"], out["failed_rows"], out["rescued_rows"] = [list(v) for v in zip(*per_call)]
    return out


def child(lib, noisy, on, a):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "%d%d" % (noisy, on), "--calls", str(a.calls), "--warmup", str(a.warmup),
           "--reps", str(a.reps), "--channels", str(a.channels), "--samples", str(a.samples), "--esn0", str(a.esn0)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


CONFIGS = (("parent_clean", True, 0, 0), ("off_clean", False, 0, 0), ("on_clean", False, 0, 1),
           ("parent_noisy", True, 1, 0), ("off_noisy", False, 1, 0), ("on_noisy", False, 1, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--benefit", action="store_true")
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--esn0", type=float, default=11.0)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(run(a, a.child[0] == "1", a.child[1] == "1")), flush=True)
        return
    if a.benefit:
        res, out = benefit(a), a.out or os.path.join(OUT_DIR, "list_benefit.json")
    else:
        out = a.out or os.path.join(OUT_DIR, "list_cost.json")
        configs = [c for c in CONFIGS if a.ab or not c[1]]
        rounds = []
        for _ in range(a.rounds):
            rounds.append({name: child(os.path.abspath(a.ab) if parent else None, noisy, on, a) for name, parent, noisy, on in configs})
            print(json.dumps(rounds[-1]), flush=True)
        summary = {}
        for inp in ("clean", "noisy"):
            names = [n for n, _, _, _ in configs if n.endswith(inp)]
            s = {}
            for mode in ("two_stream", "one_stream"):
                med = {n: [r[n][mode]["ms_per_call_median"] for r in rounds] for n in names}
                s[mode] = {"medians_ms": med, "means_ms": {n: round(statistics.mean(v), 4) for n, v in med.items()},
                           "round_to_round_spread_ms": {n: round(max(v) - min(v), 4) for n, v in med.items()}}
            on = rounds[-1]["on_" + inp]
            s["rows"], s["failed_rows"], s["rescued_rows"] = on["rows"], on["failed_rows"], on["rescued_rows"]
            summary[inp] = s
        res = {"rounds": rounds, "summary": summary}
        print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
