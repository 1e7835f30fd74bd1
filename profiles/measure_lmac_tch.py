"""Times the circuit-mode data channels (include/ext/tetra_tch.h) beside SCH/F: 65 536 rows of TCH/4.8, TCH/2.4, TCH/7.2 and SCH/F through the
counted byte-row entry points, HIP events on the launch stream, every shape warmed up, TRIALS windows of REPS launches each (a window is
a tenth of a second of kernel time and more) -> one JSON line per kind with the median, the fastest and the slowest window.

    python profiles/measure_lmac_tch.py                          this build, all four kinds
    python profiles/measure_lmac_tch.py --ab OTHER_LIB [ROUNDS]  SCH/F on this build and on another build of the library (the parent
                                                                 commit's), alternating, a fresh process per measurement: the run-to-run
                                                                 spread of each and the difference of the medians

A library given by TETRA_DEMOD_LIB (what --ab sets for its children) that lacks the TCH entry points is timed on SCH/F alone."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, TRIALS, REPS = 65536, 9, 1000


def measure(only_schf):
    import torch
    sys.path.insert(0, ROOT)
    import tetra_amd
    lb = tetra_amd.pkg.lmac_binding
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    s = torch.cuda.current_stream(dev)
    rows = torch.randint(0, 2, (N, 432), dtype=torch.uint8, device=dev, generator=g)
    si = torch.randint(0, 2 ** 31, (N,), dtype=torch.int64, device=dev, generator=g).to(torch.int32)
    ok = torch.zeros(N, dtype=torch.int32, device=dev)
    have_tch = hasattr(lb, "TCH_ABI") and hasattr(lb._lib(), "tetra_lmac_decode_tch_counted_device") and not only_schf
    kinds = [("SCH/F", lb.TPSAP_T_SCH_F, 288, False)]
    if have_tch:
        kinds += [("TCH/4.8", lb.T_TCH_4_8, 292, True), ("TCH/2.4", lb.T_TCH_2_4, 148, True), ("TCH/7.2", lb.T_TCH_7_2, 432, True)]
    result = {}
    for name, kind, n2, tch in kinds:
        ost = (n2 + 7) & ~7             # rows 8 bytes apart: the wide write-back (292 -> 296, 148 -> 152), as the frame decoder's jobs have them
        out = torch.zeros((N, ost), dtype=torch.uint8, device=dev)

        def launch():
            if tch:
                lb.decode_tch_counted_device(kind, rows, N, None, 432, si, None, out, ost, None, s)
            else:
                lb.decode_counted_device(kind, rows, N, None, 432, si, None, out, ost, ok, s)
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
        result[name] = {"rows": N, "out_stride": ost,"us_median": round(1e3 * statistics.median(ms), 2), "us_min": round(1e3 * min(ms), 2), "us_max": round(1e3 * max(ms), 2),
                        "trellis_steps": 0 if name == "TCH/7.2" else n2 + 4}
        print(json.dumps(dict(kind=name, lib=os.environ.get("TETRA_DEMOD_LIB", "this build"), **result[name])), flush=True)
    return result


def child(lib):
    env = dict(os.environ)
    env.pop("TETRA_DEMOD_LIB", None)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--schf"], env=env, capture_output=True, text=True, timeout=300, check=True)
    return json.loads(r.stdout.strip().splitlines()[-1])["us_median"]


def main():
    if "--ab" in sys.argv:
        at = sys.argv.index("--ab")
        other = os.path.abspath(sys.argv[at + 1])
        rounds = int(sys.argv[at + 2]) if len(sys.argv) > at + 2 else 5
        this, that = [], []
        for r in range(rounds):             # whichever runs first in a round changes from round to round
            if r % 2 == 0:
                this.append(child(None))
                that.append(child(other))
            else:
                that.append(child(other))
                this.append(child(None))
        print(json.dumps({"kind": "SCH/F", "rows": N, "this_build_us": this, "other_build_us": that,
                          "this_median": statistics.median(this), "other_median": statistics.median(that),
                          "this_spread": round(max(this) - min(this), 2), "other_spread": round(max(that) - min(that), 2),
                          "difference_of_medians": round(statistics.median(this) - statistics.median(that), 2)}))
        return
    measure("--schf" in sys.argv)


if __name__ == "__main__":
    main()
