"""What the AACH's soft maximum-likelihood decoding gains and costs in the receive chain (include/ext/tetra_aach_soft.h,
TETRA_RX_FLAG_AACH_SOFT).

    python profiles/measure_aach_soft.py --gain [--esn0 11]
        One second (36 000 samples) of five coded downlinks at Es/N0 = 11 dB (the stream of profiles/measure_list.py and DESIGN.md 8.3:
        seeds 9000 + c / 9100 + c, cells (300 + c, 2000 + c, 1 + c)) whose AACHs are RM(30,14) codewords (rng 9050 + c), through three
        chains on the GPU: TETRA_RX_FLAG_SOFT alone (the AACH passed through), with TETRA_RX_FLAG_AACH_RM3014, with TETRA_RX_FLAG_AACH_SOFT.
        Of the AACH rows behind a channel's first good SYNC PDU (a row's slot from its bit number, tests/aach_soft_pipeline.slots_of): rows
        equal to the sent codeword, accepted but wrong, refused; the margin histograms of ML's right and wrong rows; and the smallest
        min_margin at which ML accepts no more wrong rows than the radius-3 rule.  One seed per table.
    python profiles/measure_aach_soft.py --ab PARENT_LIB [--rounds 2]
        profiles/measure_aach_rm.py's cost measurement (4096 channels x 36 000 samples per call, two streams and one) on three builds
        in fresh processes in alternation: a build of the parent commit with TETRA_RX_FLAG_SOFT, this build with TETRA_RX_FLAG_SOFT,
        this build with TETRA_RX_FLAG_SOFT | TETRA_RX_FLAG_AACH_SOFT.
Both write into profiles/r22/aach_soft.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "r22", "aach_soft.json")
FLAG_AACH_RM3014, FLAG_SOFT, FLAG_AACH_SOFT = 2, 8, 1024


def gain(a):
    import numpy as np
    import torch  # noqa: F401 (before the library: tests/conftest.py)
    import tetra_amd
    from tests import aach_soft_definition as A
    from tests import aach_soft_pipeline as P
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    n_slots = a.samples // 510 + 2
    sent = np.stack([np.random.default_rng(9050 + c).integers(0, 16384, n_slots) for c in range(5)])
    iq = []
    for c in range(5):
        bits = pkg.synth.gen_downlink(n_slots, 9000 + c, cell=(300 + c, 2000 + c, 1 + c), aach=A.code_bits()[sent[c]])[0]
        iq.append(pkg.synth.gen_channel(a.samples, 9100 + c, bits=bits, esn0_db=a.esn0)[0].astype(np.complex64))
    iq = np.stack(iq)
    res = {"esn0_db": a.esn0, "channels": 5, "samples": a.samples, "slots_sent": int(5 * n_slots), "decoders": {}}
    for name, flags in (("pass_through", FLAG_SOFT), ("aach_rm3014", FLAG_SOFT | FLAG_AACH_RM3014), ("aach_soft", FLAG_SOFT | FLAG_AACH_SOFT)):
        rx = pkg.RxChain(5, a.samples, flags=flags)
        rx.process(iq)
        rx.wait()
        blocks, t1 = rx.fetch(R.KIND_BBK)
        margin = rx.fetch_aach_margin() if flags & FLAG_AACH_SOFT else None
        rx.close()
        label = np.stack([blocks["channel"], blocks["bitnum"], blocks["tdma_time_rx"], blocks["tdma_time"]], axis=1).astype(np.int64)
        post = (label[:, 3] >> 16) != 0
        want = A.code_bits()[sent[label[post, 0], P.slots_of(label, n_slots)[post]]]
        right = (t1[post][:, :30] == want).all(axis=1)
        ok = blocks["crc_ok"][post] != 0
        d = {"aach_rows": int(len(blocks)), "rows_behind_first_good_sync": int(post.sum()), "equal_to_sent": int((right & ok).sum()),
             "accepted_but_wrong": int((~right & ok).sum()), "refused": int((~ok).sum()), "refused_though_right": int((right & ~ok).sum())}
        if margin is not None:
            m = margin[post].astype(int)
            edges = [0, 1, 8, 16, 24, 32, 48, 64, 96, 128, 256]
            d["margin_histogram_edges"] = edges
            d["margin_histogram_right"] = [int(x) for x in np.histogram(m[right], bins=edges)[0]]
            d["margin_histogram_wrong"] = [int(x) for x in np.histogram(m[~right], bins=edges)[0]]
            d["margin_min_right"], d["margin_max_wrong"] = int(m[right].min()), int(m[~right].max()) if (~right).any() else None
            d["_margins_wrong"] = sorted(int(x) for x in m[~right])
        res["decoders"][name] = d
        print(name, json.dumps(d), flush=True)
    rm_wrong = res["decoders"]["aach_rm3014"]["accepted_but_wrong"]
    wrong = res["decoders"]["aach_soft"].pop("_margins_wrong")
    res["default_min_margin"] = next(mm for mm in range(1, 932) if sum(1 for x in wrong if x >= mm) <= rm_wrong)
    return res


def run_cost(a, which):
    import numpy as np
    import torch
    import tetra_amd
    from profiles import measure_aach_rm as M
    pkg = tetra_amd.pkg
    R = pkg.rx_binding
    d_iq = torch.from_numpy(M.stream(pkg, np, a.channels, a.samples)).cuda()
    fl = FLAG_SOFT | (FLAG_AACH_SOFT if which == 2 else 0)
    return {"flags": fl, "channels": a.channels, "samples": a.samples, "calls_per_measurement": a.calls, "reps": a.reps,
            "two_stream": M.measure(pkg, torch, d_iq, a.channels, a.samples, fl, a.calls, a.warmup, a.reps),
            "one_stream": M.measure(pkg, torch, d_iq, a.channels, a.samples, fl | R.FLAG_ONE_STREAM, a.calls, a.warmup, a.reps)}


def child(lib, which, a):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(which), "--calls", str(a.calls), "--warmup", str(a.warmup), "--reps", str(a.reps),
           "--channels", str(a.channels), "--samples", str(a.samples)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError("measurement process failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gain", action="store_true")
    ap.add_argument("--esn0", type=float, default=11.0)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=36000)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ab", default=None, metavar="PARENT_LIB")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    if a.child is not None:
        print(json.dumps(run_cost(a, a.child)), flush=True)
        return
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.gain:
        res["gain_%gdB" % a.esn0] = gain(a)
        print(json.dumps(res["gain_%gdB" % a.esn0]), flush=True)
    if a.ab:
        rounds = []
        for _ in range(a.rounds):          # fresh processes: parent, this build flag off, this build flag on, in alternation
            rounds.append({"parent_soft": child(os.path.abspath(a.ab), 1, a), "soft": child(None, 1, a), "soft_aach_soft": child(None, 2, a)})
            print(json.dumps(rounds[-1]), flush=True)
        summary = {}
        for mode in ("two_stream", "one_stream"):
            med = {k: [r[k][mode]["ms_per_call_median"] for r in rounds] for k in ("parent_soft", "soft", "soft_aach_soft")}
            mean = {k: statistics.mean(v) for k, v in med.items()}
            summary[mode] = {"medians_ms": med, "parent_round_to_round_spread_ms": round(max(med["parent_soft"]) - min(med["parent_soft"]), 4),
                             "flag_off_minus_parent_ms": round(mean["soft"] - mean["parent_soft"], 4),
                             "flag_on_minus_flag_off_ms": round(mean["soft_aach_soft"] - mean["soft"], 4)}
        summary["decode_stage_ms"] = {k: [r[k]["one_stream"]["stage_ms"][3] for r in rounds] for k in ("parent_soft", "soft", "soft_aach_soft")}
        res["three_builds"] = {"rounds": rounds, "summary": summary}
        print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
