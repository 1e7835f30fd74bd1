"""Cost of the frequency-shifted channeliser (include/tetra_shift.h) on config 5's geometry: 5e6 wideband samples -> 12500 frames x
800 channels (M 800, P 8, D 400), complex64 and cs16, k_channelise_fft un-shifted and with half a bin of shift; HIP events on the
launch stream (tetra_chan_last_kernel_ms), 30 warm-up and 40 timed launches per variant, alternating, median.

    python profiles/measure_chan_shift.py [--baseline-lib OLD.so] [--rounds 3] [--swap] [--flags 1] [--out profiles/r09/chan_shift.json]

Every round is a fresh process per library (the tree's, then --baseline-lib: a build of the parent commit, same ABI), alternating, so
the two are compared on the same machine in the same session; the spread of the tree's un-shifted medians over the rounds is the
run-to-run noise the comparison is read against.  --swap runs the baseline in front of the tree in every round.  --flags: the
channeliser's create flags (1 = TETRA_CHAN_FLAG_VALU_DFT: k_channelise, 2 = TETRA_CHAN_FLAG_MATRIX_DFT: k_channelise_mfma instead
of k_channelise_fft), same workload."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, P, D, N_IN = 800, 8, 400, 5000000


def worker(flags):
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    dev = torch.device("cuda", 0)
    n_in = N_IN
    frames = n_in // D
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    x = torch.view_as_complex(torch.randn((n_in, 2), device=dev, generator=g)).contiguous()
    xs = torch.view_as_real(x).mul(32768.0 / 6).round().clamp(-32768, 32767).to(torch.int16).contiguous()
    s = torch.cuda.current_stream(dev)
    has_shift = hasattr(pkg.load_library(), "tetra_chan_set_shift")
    half = (1 << 32) // 1600
    variants = {"unshifted": 0}
    if has_shift:
        variants["shifted"] = half
    out = torch.zeros((frames, M), dtype=torch.complex64, device=dev)
    res = {}
    for fmt, src in (("complex64", x), ("cs16", xs)):
        chs = {}
        for name, inc in variants.items():
            chs[name] = pkg.Channeliser(M, P, D, max_in=n_in, flags=flags)
            if inc:
                chs[name].set_shift(inc)
        for _ in range(30):
            for ch in chs.values():
                ch.process_device(src, n_in, out, s)
        torch.cuda.synchronize()
        ms = {k: [] for k in chs}
        for _ in range(40):
            for k, ch in chs.items():
                ch.process_device(src, n_in, out, s)
                torch.cuda.synchronize()
                ms[k].append(ch.last_kernel_ms())
        res[fmt] = {k: {"median_ms": round(sorted(v)[len(v) // 2], 5), "min_ms": round(min(v), 5)} for k, v in ms.items()}
        for ch in chs.values():
            ch.close()
    print("RESULT " + json.dumps(res))


def run(lib, flags=0):
    env = dict(os.environ)
    if lib:
        env["TETRA_DEMOD_LIB"] = lib
    else:
        env.pop("TETRA_DEMOD_LIB", None)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--flags", str(flags)], env=env, capture_output=True, text=True, timeout=280)
    if p.returncode != 0:
        raise SystemExit("worker failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--swap", action="store_true")
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09", "chan_shift.json"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.flags)
    tree, base = [], []
    for _ in range(a.rounds):
        if a.baseline_lib and a.swap:
            base.append(run(os.path.abspath(a.baseline_lib), a.flags))
        tree.append(run(None, a.flags))
        if a.baseline_lib and not a.swap:
            base.append(run(os.path.abspath(a.baseline_lib), a.flags))
    n_in = N_IN
    doc = {"workload": "%d samples -> %d frames x %d channels, P %d, flags %d, %s first" % (n_in, n_in // D, M, P, a.flags, "parent" if a.swap else "tree"), "rounds": {"tree": tree, "parent": base}}
    for fmt in ("complex64", "cs16"):
        u = [r[fmt]["unshifted"]["median_ms"] for r in tree]
        sh = [r[fmt]["shifted"]["median_ms"] for r in tree]
        d = {"unshifted_ms": min(u), "unshifted_ms_rounds": u, "noise_rel": round((max(u) - min(u)) / min(u), 4), "shifted_ms": min(sh),
             "shifted_over_unshifted": round(min(sh) / min(u), 4)}
        if base:
            b = [r[fmt]["unshifted"]["median_ms"] for r in base]
            bs = [r[fmt]["shifted"]["median_ms"] for r in base]
            d.update(parent_ms=min(b), parent_ms_rounds=b, unshifted_over_parent=round(min(u) / min(b), 4), shifted_ms_rounds=sh,
                     parent_shifted_ms_rounds=bs)
        doc[fmt] = d
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps({k: doc[k] for k in ("complex64", "cs16")}))


if __name__ == "__main__":
    main()
