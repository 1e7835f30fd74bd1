"""What the retune with a donor (include/ext/tetra_handover.h) gains and costs.

  --first-block   tests/restart_gpu.py's band (one base station on 32 bins: control carrier A, traffic carrier B with one SYNC burst per
                  multiframe, 0.25 s calls, slot 1 moved onto B just behind B's SYNC burst) at Es/N0 25, 20 and 11 dB: slot periods from the
                  move to the moved slot's first CRC-good NDB or SCH/F block with a donor, its hand-over status, and the same for the plain
                  retune (B's next SYNC burst is 70.4 slot periods after the move; the capture ends 78 after it)
  --cost          profiles/measure_retune.py's schedule (20 MHz cs16 capture in 0.25 s blocks, 16 coded downlinks, ms per block between
                  two HIP events, median over --reps) for: no retune on a handle that never handed over (`none`); one slot moved before
                  every block plainly (`one`) and with its neighbour as donor (`one_from`); no retune on a handle that has handed over once,
                  i.e. the ASSIST-capable synchroniser kernel and the apply kernel in every tail (`none_after`)

    python profiles/measure_handover.py --first-block --cost          # -> profiles/r21/handover.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

OUT = os.path.join(ROOT, "profiles", "r21", "handover.json")


def first_block(pkg, torch):
    from tests import restart_gpu as T
    R = pkg.rx_binding
    moved = [T.BIN_A, T.BIN_B2, T.BIN_B]
    traffic = (R.KIND_NDB1, R.KIND_NDB2, R.KIND_SCH_F)
    move_bit = T.CALL * 36000 // 800000
    out = {"move_at_slot": round(move_bit / 510, 2), "next_sync_burst_of_B_at_slot": T.B_SYNC_SLOTS[2], "capture_slots": T.N_SLOTS, "by_esn0": {}}
    for esn0 in (25.0, 20.0, 11.0):
        xs = T.band_capture(torch, pkg.synth, esn0_db=esn0)
        row = {}
        for name, donors in (("with_donor", [-1, 0, -1]), ("plain", None)):
            wb = pkg.WidebandRx([T.BIN_A, T.BIN_EMPTY, T.BIN_B], n_channels=T.M_BAND, decimation=T.D_BAND, max_in=T.CALL)
            snaps, status = T.drive(pkg, torch, wb, xs, T.band_calls(xs.shape[0]), {1: lambda w: w.retune(moved, donors=donors)})
            rows = [(r[1], k) for s in snaps[1:] for k in traffic for r in s[1]["rows"][k] if r[2]]
            all_rows = sum(len(s[1]["rows"][k]) for s in snaps[1:] for k in traffic)
            wit = sum(1 for s in snaps[1:] for k in traffic for r in s[2]["rows"][k] if r[2])
            row[name] = {"handover_status": list(status[-1][1]), "traffic_blocks": all_rows, "traffic_blocks_crc_good": len(rows),
                         "witness_traffic_blocks_crc_good": wit,
                         "first_crc_good_traffic_block_slot_periods_after_the_move": round(min(rows)[0] / 510, 2) if rows else None}
            wb.close()
        out["by_esn0"]["%g" % esn0] = row
        print(esn0, json.dumps(row), flush=True)
        del xs
    return out


def cost(pkg, torch, n_blocks, warmup, reps, capture_blocks):
    from measure_wbrx import BINS, BLOCK, capture
    R = pkg.rx_binding
    xs = capture(torch, pkg.synth, capture_blocks)
    blk = [xs[b * BLOCK:(b + 1) * BLOCK] for b in range(xs.shape[0] // BLOCK)]
    s = torch.cuda.current_stream()
    res = {}
    for mode in ("none", "one", "one_from", "none_after", "none", "one", "one_from", "none_after"):
        bins = list(BINS)
        wb = pkg.WidebandRx(bins, max_in=BLOCK)
        step = [0]

        def block():
            i = step[0]
            step[0] += 1
            if mode in ("one", "one_from"):          # measure_retune.py's mode `one`; the donor is the next slot, which stays in this block
                j = i % 16
                bins[j] = (BINS[j] + 20) % 800 if bins[j] == BINS[j] else BINS[j]
                wb.retune(bins, s, donors=[(k + 1) % 16 for k in range(16)] if mode == "one_from" else None)
            wb.process_device(blk[i % len(blk)], BLOCK, s)

        if mode == "none_after":                    # one hand-over, then the schedule of `none`
            wb.process_device(blk[0], BLOCK, s)
            moved = list(BINS)
            moved[0] = (BINS[0] + 20) % 800
            wb.retune(moved, s, donors=[1] * 16)
            wb.process_device(blk[1], BLOCK, s)
            wb.retune(list(BINS), s)
        for _ in range(warmup):
            block()
        wb.rx.wait()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(n_blocks):
                block()
            wb.rx.rows_device(R.KIND_SB1, 0, s)
            e1.record(s)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / n_blocks)
        states = [st[0] for st in wb.handover_status()]
        res.setdefault(mode, []).append({"ms_per_block_median": round(statistics.median(ms), 4), "ms_per_block_min": round(min(ms), 4),
                                         "ms_per_block_max": round(max(ms), 4), "chain_stage_ms": [round(v, 4) for v in wb.rx.stage_ms()],
                                         "handover_states_at_the_end": {str(v): states.count(v) for v in sorted(set(states))}})
        print(mode, json.dumps(res[mode][-1]), flush=True)
        wb.close()
    med = {m: statistics.mean(r["ms_per_block_median"] for r in v) for m, v in res.items()}
    res["one_from_minus_one_ms"] = round(med["one_from"] - med["one"], 4)
    res["none_after_minus_none_ms"] = round(med["none_after"] - med["none"], 4)
    res["none_round_to_round_ms"] = round(abs(res["none"][0]["ms_per_block_median"] - res["none"][1]["ms_per_block_median"]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--first-block", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--capture-blocks", type=int, default=4)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    import tetra_amd
    pkg = tetra_amd.pkg
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.first_block:
        res["first_block"] = first_block(pkg, torch)
    if a.cost:
        res["cost"] = cost(pkg, torch, a.blocks, a.warmup, a.reps, a.capture_blocks)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
