"""bench.py's N > 1 path on real hardware: `python bench.py --gpus 2` by itself starts two ranks (here both mapped onto the
one GPU of the box), once over gloo and once over RCCL; on a box with fewer GPUs than ranks the line is marked functional_only
(value null, n_gpus = the GPUs that ran) and the known-answer check (a --full leg) is green.  Beside them, a plain one-rank run
carries the headline alone."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gpurun_out")


def _run(backend):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--backend", backend]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)


def _line(r):
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(lines[0])


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_bench_gpus_2_runs_two_ranks(backend):
    """`python bench.py --gpus 2 ...` alone.  With a GPU per rank the default backend is RCCL; on a box with fewer GPUs than ranks
    (both ranks on the one GPU here) RCCL would refuse the communicator ("Duplicate GPU detected"), so bench.py lines the ranks up
    over gloo and says so in the line -- either way two ranks run; a folded run can not be mistaken for a 2-GPU measurement."""
    import torch
    r = _run(backend)
    d = _line(r)
    os.makedirs(OUT, exist_ok=True)
    json.dump(d, open(os.path.join(OUT, "bench_gpus2_%s.json" % backend), "w"))
    assert d["n_ranks"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["ramp_steps"] == 8
    ngpu = torch.cuda.device_count()
    assert d["gpus_physical"] == ngpu and d["n_gpus"] == min(2, ngpu) and d["functional_only"] == (ngpu < 2)
    value = d["value"]
    if ngpu < 2:
        assert d["value"] is None and "NOT an" in d["functional_note"]
        value = d["value_functional"]
    if backend == "nccl" and torch.cuda.device_count() >= 2:
        assert d["dist_backend"] == "nccl" and d["rccl_world_size"] == 2
    else:
        assert d["dist_backend"] == "gloo" and d["rccl_world_size"] is None
        assert ("dist_backend_note" in d) == (backend == "nccl")
    assert d["check"]["bit_errors"] <= 1e-3 * d["check"]["bits_compared_last_quarter"]
    # two ranks of 4096 channels each: the whole-job value counts both
    assert abs(value - 2 * 4096 * 36000 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * value


def test_bench_gpus_4_folded_onto_the_box(tmp_path):
    """the driver's SCALE run is `bench.py --gpus 8` on an 8-GPU node that no round has had.  Here the same
    command starts FOUR ranks (512 channels each so that the handles, inputs and bit rows fit beside each other on one GPU), folded
    onto the GPUs the box has: rendezvous, several ranks' worth of barriers and the MAX / SUM reductions, a known-answer check on
    every rank -- its own channel range against its own transmitted bits -- and a line nobody can mistake for a 4-GPU measurement.
    Four ranks, not eight: with this test's own process that keeps five processes at most with the GPU open at once."""
    import torch
    import numpy as np
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1", "--channels", "512",
           "--full", "--no-cpu-baseline", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    d = _line(r)
    os.makedirs(OUT, exist_ok=True)
    json.dump(d, open(os.path.join(OUT, "bench_gpus4_folded.json"), "w"))
    ngpu = torch.cuda.device_count()
    assert d["n_ranks"] == 4 and d["gpus_physical"] == ngpu and d["n_gpus"] == min(4, ngpu) and d["scaling"] == "weak"
    assert d["functional_only"] == (ngpu < 4)
    if ngpu < 4:
        assert d["value"] is None and d["value_functional"] > 0 and "NOT an 4-GPU measurement" in d["functional_note"]
        assert d["dist_backend"] == "gloo" and "RCCL needs one GPU per rank" in d["dist_backend_note"]
    ck = d["check"]
    assert ck["ranks_checked"] == 4 and ck["ranks_green"] == 4 and ck["channels_checked"] == 4 * 256          # bench.CHECK_CHANNELS of every rank
    assert ck["bit_errors"] <= 1e-3 * ck["bits_compared_last_quarter"] and ck["bits_compared_last_quarter"] > 4 * 32 * 8000
    assert d["config"]["channels_per_gpu"] == 512
    # --dump-outputs with N > 1: every rank's part gathered, ONE set for the whole bank (global channel numbers) under the names the
    # line reports, within 64 MB
    dd = d["dump_outputs"]
    assert sorted(os.listdir(dump)) == [n + ".npy" for n in dd["arrays"]] == ["bits.npy", "bits_channels.npy", "n_bits.npy"]
    assert dd["bytes"] == sum(os.path.getsize(dump / f) for f in os.listdir(dump)) <= 64 << 20
    rows, sel, nb = (np.load(dump / (n + ".npy")) for n in dd["arrays"])
    assert nb.shape == (4 * 512,) and (np.abs(nb - 36000) < 360).all() and rows.shape[0] == dd["rows"] == 256
    assert [int((sel // 512 == q).sum()) for q in range(4)] == [64] * 4 and np.array_equal(sel, np.unique(sel))
    for j, c in enumerate(sel.astype(np.int64)):
        assert (rows[j, : int(nb[c])] >= 0).all() and (rows[j, int(nb[c]):] == -1).all()


def test_bench_rccl_half_of_the_rank_path_on_one_gpu():
    """RCCL refuses several ranks on one device, so on a one-GPU box its half of bench.py's N > 1 path -- communicator set-up
    with device_id, barrier, MAX all-reduce of the elapsed time on a device tensor, tear-down -- runs as a ONE-rank group
    (--force-dist); the two-rank half runs over gloo above."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
           "--no-host-path", "--no-large-batch", "--no-config5", "--no-time-major", "--force-dist", "--backend", "nccl"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    d = _line(r)
    os.makedirs(OUT, exist_ok=True)
    json.dump(d, open(os.path.join(OUT, "bench_force_dist_nccl.json"), "w"))
    assert d["n_gpus"] == 1 and d["dist_backend"] == "nccl" and d["rccl_world_size"] == 1
    assert d["check"]["bit_errors"] <= 1e-3 * d["check"]["bits_compared_last_quarter"]


def test_bench_under_the_driver_s_own_launcher():
    """The driver's command line for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...` -- bench.py then runs as ONE of the ranks (it must not start ranks of its own)."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--full", "--no-cpu-baseline", "--backend", "gloo"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    d = _line(r)
    import torch
    assert d["n_ranks"] == 2 and d["n_gpus"] == min(2, torch.cuda.device_count()) and d["dist_backend"] == "gloo"
    assert d["functional_only"] == (torch.cuda.device_count() < 2)
    # 256 channels per rank from their own seeds at 25 dB: a few true channel errors among millions of bits (bench.py's own bound)
    assert d["check"]["bit_errors"] <= 1e-3 * d["check"]["bits_compared_last_quarter"]


def test_chain_leg_known_answer_at_full_size():
    """The receive chain at BASELINE's size through the one property that does not need the reference beside it: 4096 channels x 36000
    samples of CODED downlinks (the reference's encoder chain restated in synth.gen_downlink, pinned on the reference's own encoder
    by tests/test_synth_tx.py) -> tetra_rx -> every one of the ~651 000 blocks of the checked call has a good CRC, every block of
    the 64 distinct streams carries exactly the type-1 bits sent in the slot its TDMA label names, every channel is locked and reads
    its cell -- on two streams and on one (`bench.py --chain-only` fails the run otherwise; the counters are asserted here too)."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--chain-only"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(OUT, exist_ok=True)
    json.dump(d, open(os.path.join(OUT, "bench_chain_only.json"), "w"))
    ck = d["check"]
    assert ck["channels"] == 4096 and ck["channels_locked"] == 4096 and ck["cells_read"] == 4096
    total = 0
    for nm, c in ck["blocks"].items():
        assert c["rows"] == c["crc_good"] > 60000 and c["checked_rows"] == c["type1_bits_and_tdma_slot_exact"] > 1000, (nm, c)
        total += c["rows"]
    assert total > 600000 and d["rows_per_kind"]["schf"] == ck["blocks"]["schf"]["rows"]
    assert 3.5 < d["two_streams_ms_per_second"] < d["one_stream_ms_per_second"] * 1.02 < 6.0        # sanity: not a timing claim
    assert set(d["stages_one_stream"]) == {"demodulator", "burst_sync", "frame_lists_sb1_decode_track", "other_kinds_decode_label"}


def test_bench_dump_outputs_are_the_same_on_a_second_run(tmp_path):
    """`bench.py --dump-outputs DIR`: two runs with the same arguments dump the same arrays (same inputs, same last timed step), and
    what is dumped is the call's output -- the counts are those of two demodulated seconds at 36 ksps.  At twice the headline samples a
    row is twice as long: fewer rows are sampled, the files stay within 64 MB."""
    import numpy as np
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--channels", "512",
            "--samples", "72000", "--full", "--no-cpu-baseline", "--no-host-path", "--no-large-batch", "--no-config5", "--no-time-major",
            "--no-chain"]
    got = []
    for k in range(2):
        d = tmp_path / ("d%d" % k)
        r = subprocess.run(base + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        line = _line(r)
        dd = line["dump_outputs"]
        assert line["steps"] == 3 and line["ms_per_step"] > 0 and dd["arrays"] == ["bits", "bits_channels", "n_bits"]
        assert dd["bytes"] == sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20 and 128 < dd["rows"] < 256
        got.append({n: np.load(d / (n + ".npy")) for n in dd["arrays"]})
    for n in got[0]:
        assert got[0][n].dtype == got[1][n].dtype and np.array_equal(got[0][n], got[1][n]), n
    nb, rows = got[0]["n_bits"], got[0]["bits"]
    assert nb.shape == (512,) and rows.shape[0] == got[0]["bits_channels"].shape[0] and (np.abs(nb - 72000) < 720).all()
    assert set(np.unique(rows)) <= {-1.0, 0.0, 1.0} and 0.4 < (rows == 1).sum() / (rows >= 0).sum() < 0.6


def test_plain_run_is_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: set-up, ramp, warm-up, the K timed steps, --dump-outputs and the line --
    the contract fields and the roofline of the timed launches, but no known-answer check, CPU baseline or informational leg (those
    are --full's)."""
    import numpy as np
    dump = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    d = _line(r)
    assert d["full"] is False and d["check"] is None and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["metric"] == "IQ Msamples/s demodulated to bits, batched TETRA channels" and d["unit"] == "Msamples/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["roofline"]["kernel_ms"] > 0
    assert abs(d["value"] - 4096 * 36000 / (d["ms_per_step"] * 1e-3) / 1e6) < 1e-3 * d["value"]
    legs = {"cpu_baseline", "cpu_baseline_fast", "time_major", "large_batch", "config5", "chain"}
    assert not legs & set(d) and not [k for k in d if k.startswith("host_path")], sorted(d)
    dd = d["dump_outputs"]
    assert dd["arrays"] == ["bits", "bits_channels", "n_bits"] and dd["rows"] == 256
    nb = np.load(dump / "n_bits.npy")
    assert nb.shape == (4096,) and (np.abs(nb - 36000) < 360).all()
