#!/usr/bin/env python3
"""Which kernels a demodulator handle launches, case by case: the evidence behind tests/golden/demod_launch_plan.json.

All workgroup shapes give the same bits, so no parity test can see a wrong launch plan (csrc/launch_plan.hpp).  This script creates
one handle per case of a fixed matrix (channels x create flags x design, plus handles moved by the setters), runs ONE 64-sample
tetra_demod_process_device on each and prints the case list as JSON.  Run under a kernel trace, the trace then says what each case
launched:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o plan -- python profiles/trace_launch_plan.py --cases OUT/cases.json
    python profiles/trace_launch_plan.py --extract OUT/cases.json OUT/**/plan_kernel_trace.csv > tests/golden/demod_launch_plan.json

Every successful create launches k_fill_* kernels (the state reset) and every process call k_fused / k_generic ones, all in
program order on the null stream: the demodulator launches between one case's fills and the next one's are that case's.
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAX_SAMPLES, N = 256, 64
CHANNELS = [1, 4, 5, 16, 17, 800, 1024, 1025, 4096, 4112, 8192, 8208, 12288, 16400]
FLAGS = {"0": 0, "WIDE": 16, "NARROW": 32, "SMALL": 64, "GENERIC_KERNEL": 128}
DESIGNS = [
    ("default", {}),
    ("taps69", dict(rrc_tap_count=69)),                                 # above the 32-channel shape's 68, within the regular rows' 72
    ("taps81", dict(rrc_tap_count=81)),                                 # long rows
    ("taps129", dict(rrc_tap_count=129)),
    ("deep1", dict(samplerate=18000.0)),                                # timing loop below one sample per symbol
    ("deep1_taps81", dict(samplerate=18000.0, rrc_tap_count=81)),       # ... with long rows: the only way to k_fused<.., 1, true>
    ("deep2", dict(samplerate=18000.0 * 0.2)),                          # ... below 0.27
    ("deep2_taps81", dict(samplerate=18000.0 * 0.2, rrc_tap_count=81)),
    ("generic", dict(samplerate=18000.0 * 0.06)),                       # ... below 0.07: the generic kernel's domain
]
# a default handle moved by a setter: it must plan like a fresh handle of that design
SETTERS = [
    dict(design="deep2", channels=4096, flags=0, setter="set_param"),
    dict(design="taps81", channels=800, flags=0, setter="set_rrc_params"),
    dict(design="taps81", channels=4096, flags=0, setter="set_tables"),
]


def cases():
    out = [dict(design=dname, channels=ch, flags=fl) for dname, _ in DESIGNS for ch in CHANNELS for fl in FLAGS.values()]
    return out + [dict(s) for s in SETTERS]


def run(path):
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    B = pkg.binding
    _, cus = B.device_info(0)
    cmax = max(CHANNELS)
    g = torch.Generator(device="cuda").manual_seed(1)
    iq = torch.randn(cmax * N * 2, device="cuda", generator=g) * 0.1
    nb = torch.zeros(cmax, dtype=torch.int32, device="cuda")
    bits = torch.zeros(1, dtype=torch.uint8, device="cuda")
    long_tables = None
    torch.cuda.synchronize()
    done = []
    for c in cases():
        rec = dict(c, cus=cus)
        prm = dict(DESIGNS)[c["design"]]
        try:
            if c.get("setter"):
                if c["setter"] == "set_tables" and long_tables is None:      # tables of a fresh 81-tap handle, fetched before this case starts
                    t = pkg.Demodulator(1, MAX_SAMPLES, device=0, **prm)
                    long_tables = t.tables()
                    t.close()
                d = pkg.Demodulator(c["channels"], MAX_SAMPLES, device=0, flags=c["flags"])
                if c["setter"] == "set_param":
                    for k, v in prm.items():
                        d.set_param(k, v)
                elif c["setter"] == "set_rrc_params":
                    d.set_rrc_params(prm["rrc_tap_count"], 0.35)
                else:
                    d.set_tables(rrc_taps=long_tables["rrc"], bandedge_taps=[long_tables["be_re"], long_tables["be_im"]])
            else:
                d = pkg.Demodulator(c["channels"], MAX_SAMPLES, device=0, flags=c["flags"], **prm)
        except B.TetraDemodError as e:
            rec["status"] = e.status      # refused combinations are recorded, not dropped
            done.append(rec)
            continue
        rec["status"] = 0
        stride = d.bits_stride(N)
        if bits.numel() < c["channels"] * stride:
            bits = torch.zeros(c["channels"] * stride, dtype=torch.uint8, device="cuda")
        d.process_device(iq, N, bits, stride, nb)
        torch.cuda.synchronize()
        d.close()
        done.append(rec)
    with open(path, "w") as f:
        json.dump(done, f)
    print(json.dumps(done))


def extract(cases_path, trace_path):
    with open(cases_path) as f:
        recs = json.load(f)
    with open(trace_path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    groups, in_fill = [], False
    for r in rows:
        name = r["Kernel_Name"]
        if "k_fill_" in name:
            if not in_fill:
                groups.append([])
            in_fill = True
            continue
        m = re.search(r"k_fused<[^>]*>|k_generic", name)
        if not m:
            continue
        in_fill = False
        wg = int(r["Workgroup_Size_X"])
        groups[-1].append([m.group(0).replace(" ", ""), int(r["Grid_Size_X"]) // wg, wg])      # kernel, workgroups, workgroup size
    groups = [g for g in groups if g]       # (a handle created only to fetch tables launches nothing)
    ok = [r for r in recs if r["status"] == 0]
    if len(groups) != len(ok):
        raise SystemExit("%d launch groups in the trace for %d created handles" % (len(groups), len(ok)))
    for r, g in zip(ok, groups):
        r["launches"] = g
    for r in recs:
        r.setdefault("launches", [])
    head = dict(max_samples=MAX_SAMPLES, n_samples=N, flag_names=FLAGS, designs=dict(DESIGNS))
    print("{" + ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in head.items()) + ',\n"cases": [\n' +
          ",\n".join(json.dumps(r) for r in recs) + "\n]}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="launch_plan_cases.json", help="where the run writes its case records")
    ap.add_argument("--extract", nargs=2, metavar=("CASES", "TRACE_CSV"), help="merge a run's case records with its kernel trace: the fixture, on stdout")
    a = ap.parse_args()
    if a.extract:
        extract(*a.extract)
    else:
        run(a.cases)
