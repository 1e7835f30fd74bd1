"""The wideband receiver (include/tetra_wbrx.h): one SDR capture in, the receive chain's blocks per carrier out.

It is the composition of pinned stages -- channeliser (tetra_chan.h), resampler (tetra_resamp_*), receive chain (tetra_rx.h) -- with
one new kernel, the resampler over picked columns.  The tests hold the handle bit for bit against the hand-wired composition of the
existing handles, and the picking thread code against the full resampler's on the host."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.chain_gpu import bit_rows as _bit_rows, collect
from tests.wideband_gpu import capture as _capture, cs16 as _cs16  # noqa: F401  (other test modules take them from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE, ERR_SIZE, ERR_ALIGN = -1, -3, -6, -7


# ---------------------------------------------------------------------------------------------------------------------- CPU


def test_wbrx_header_symbols_all_exported(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tetra_wbrx.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tetra_wbrx_[a-z0-9_]+)\s*\(", src)))
    L = pkg.load_library()
    assert set(names) == set(pkg.wbrx_binding.WBRX_EXPORTS) and len(names) == 14
    for n in names:
        assert hasattr(L, n), n


def test_wbrx_config_layout_matches_header(pkg):
    fields = ["chan", "interp", "decim", "taps_per_phase", "n_bins", "resamp_cutoff_rel", "resamp_kaiser_beta", "bins", "rx"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "tetra_wbrx.h"\nint main(){printf("%zu", sizeof(tetra_wbrx_config_t));' +
            "".join('printf(" %%zu", offsetof(tetra_wbrx_config_t, %s));' % f for f in fields) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        cfile = os.path.join(td, "s.c")
        open(cfile, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)
        got = list(map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()))
    W = pkg.wbrx_binding.WbrxConfig
    assert got == [C.sizeof(W)] + [getattr(W, f).offset for f in fields]


def test_wbrx_default_config(pkg):
    cfg = pkg.wbrx_binding.default_config()
    assert (cfg.chan.n_channels, cfg.chan.taps_per_channel, cfg.chan.decimation) == (800, 8, 400)
    assert (cfg.interp, cfg.decim, cfg.taps_per_phase, cfg.n_bins, cfg.bins) == (18, 25, 16, 0, None)
    assert (cfg.rx.demod.n_channels, cfg.rx.demod.max_samples, cfg.rx.demod.layout, cfg.rx.kinds) == (0, 0, 1, 0)


def test_wbrx_no_cpu_fallback(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.TetraDemodError) as e:
        pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16)
    assert e.value.status == ERR_NO_DEVICE


def _picking_cases():
    """Every triple of the product's table of specialised ratios (read from it through the emulation library, resamp_core.hpp) at M
    = 32, the default ratio on the 800 bins of config 5, and two generic cases."""
    from tests.emul import resamp_emul_bind as re_
    return [(32, I, DN, T, False) for I, DN, T in re_.ratios()] + [(800, 18, 25, 16, False), (32, 18, 25, 16, True), (12, 5, 7, 11, True)]


def test_ratio_table_is_the_documented_seven():
    from tests.emul import resamp_emul_bind as re_
    assert sorted(re_.ratios()) == sorted([(18, 25, 8), (18, 25, 12), (18, 25, 16), (18, 25, 24), (2, 3, 8), (3, 2, 8), (1, 2, 8)])


@pytest.mark.parametrize("M,I,DN,T,generic", _picking_cases())
def test_picking_thread_code_equals_full_resampler_then_column_pick(oracle, M, I, DN, T, generic):
    """The selecting resampler's thread code (resamp_core.hpp, PickColumns) compiled for the host over a random [frames][M] input,
    random bin subsets in random order, ragged calls (empty ones, calls shorter than one group of DN frames and than the delay line)
    equals the full resampler's host build followed by the column pick, bit for bit."""
    from tests.emul import resamp_emul_bind as re_
    proto = oracle.ResampOracle(M, I, DN, T).h
    rng = np.random.default_rng(M + I + T + int(generic))
    n = 12 * DN + 29 if M > 100 else 40 * DN + 13
    x = (rng.standard_normal((n, M)) + 1j * rng.standard_normal((n, M))).astype(np.complex64)
    for trial in range(3):
        cols = rng.permutation(M)[: int(rng.integers(1, min(M, 40) + 1))].astype(np.int32)
        full = re_.ResampEmul(M, I, DN, T, proto, generic=generic)
        pick = re_.ResampSelectEmul(M, cols, I, DN, T, proto, generic=generic)
        cuts = sorted(set([0, 0, 1, 3, DN - 1, DN + 2, T + 5, 3 * DN + 1, int(rng.integers(4 * DN, n)), n]))
        cuts = [0] + cuts + [n]
        for a, b in zip(cuts, cuts[1:]):
            yf, yp = full.process(x[a:b]), pick.process(x[a:b])
            assert yp.shape == (yf.shape[0], cols.size), (trial, a, b)
            assert np.array_equal(np.ascontiguousarray(yf[:, cols]).view(np.uint32), yp.view(np.uint32)), (trial, a, b)


# ---------------------------------------------------------------------------------------------------------------------- GPU


def _rows(rx, R, which=0):
    return collect(rx, R, which)


M_SMALL, D_SMALL, BINS_SMALL = 32, 16, [1, 7, 20, 31]
CARRIERS_SMALL = {1: 11, 7: 12, 20: 13, 31: 14}


@pytest.fixture(scope="module")
def small_capture(pkg, synth):
    import torch
    return _capture(torch, synth, M_SMALL, CARRIERS_SMALL, 80)


def _small_max_samples(max_in):
    return ((D_SMALL - 1 + max_in) // D_SMALL) * 18 // 25 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["c64", "cs16"])
def test_gpu_wbrx_equals_the_hand_wired_composition(pkg, small_capture, fmt):
    """The same capture, the same call cuts: WidebandRx against Channeliser(32) -> Resampler(32) -> column pick in torch ->
    RxChain(4, time-major).  Every kind's rows and labels, the type-1 bits, the cell and sync states, the demodulator's bit rows and the
    resampled frames are equal, bit for bit."""
    import torch
    R = pkg.rx_binding
    x, cells, tx = small_capture
    xin = x if fmt == "c64" else _cs16(torch, x)
    L = x.shape[0]
    cuts = [0, 5, 5 + 9, 200003, 200003 + 16 * 1000 + 7, 470000, 470010, 700001, L]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in)
    ch = pkg.Channeliser(M_SMALL, decimation=D_SMALL, max_in=max_in)
    rs = pkg.Resampler(M_SMALL, max_in=(D_SMALL - 1 + max_in) // D_SMALL)
    rx = pkg.RxChain(len(BINS_SMALL), _small_max_samples(max_in), layout=pkg.binding.LAYOUT_TIME_MAJOR)
    chan_buf = torch.zeros(((D_SMALL - 1 + max_in) // D_SMALL, M_SMALL), dtype=torch.complex64, device="cuda")
    res_buf = torch.zeros((_small_max_samples(max_in), M_SMALL), dtype=torch.complex64, device="cuda")
    cols = torch.tensor(BINS_SMALL, device="cuda")
    s = torch.cuda.current_stream()
    for a, b in zip(cuts, cuts[1:]):
        part = xin[a:b]
        wb.process_device(part, b - a, s)
        nf = ch.process_device(part, b - a, chan_buf, s)
        nr = rs.process_device(chan_buf, nf, res_buf, s)
        picked = res_buf[:nr][:, cols].contiguous()
        rx.process_device(picked if nr else res_buf, nr, s)          # (an empty tensor has no address)
        assert torch.equal(torch.view_as_real(wb.frames()).view(torch.int32), torch.view_as_real(picked).view(torch.int32)), (a, b)
        assert _rows(wb.rx, R) == _rows(rx, R), (a, b)
        assert _bit_rows(torch, wb.rx, 4) == _bit_rows(torch, rx, 4), (a, b)
        torch.cuda.synchronize()
    assert [bytes(c) for c in wb.rx.cells()] == [bytes(c) for c in rx.cells()]
    assert wb.rx.sync_states() == rx.sync_states()
    assert list(wb.bins()) == BINS_SMALL
    ms = wb.stage_ms()
    assert len(ms) == 2 and all(v >= 0 for v in ms)
    wb.close()
    rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [8, 24])
def test_gpu_wbrx_picked_columns_for_other_tap_counts(pkg, small_capture, T):
    """The picking kernels of the table's other two 18 / 25 lengths (the demodulator keeps its 36 ksps): tetra_wbrx_frames_device
    equals Channeliser(32) -> Resampler(32, T) -> column pick bit for bit, over one call of a few thousand samples, a ragged one
    that brings fewer frames than the picked delay line holds, and one behind it that reads that line."""
    import torch
    x = small_capture[0]
    cuts = [0, 4099, 4099 + 37, 4099 + 37 + 1000]
    max_in = 4099
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in, taps_per_phase=T)
    ch = pkg.Channeliser(M_SMALL, decimation=D_SMALL, max_in=max_in)
    rs = pkg.Resampler(M_SMALL, taps_per_phase=T, max_in=(D_SMALL - 1 + max_in) // D_SMALL)
    chan_buf = torch.zeros(((D_SMALL - 1 + max_in) // D_SMALL, M_SMALL), dtype=torch.complex64, device="cuda")
    res_buf = torch.zeros((_small_max_samples(max_in), M_SMALL), dtype=torch.complex64, device="cuda")
    cols = torch.tensor(BINS_SMALL, device="cuda")
    s = torch.cuda.current_stream()
    total = 0
    for a, b in zip(cuts, cuts[1:]):
        wb.process_device(x[a:b], b - a, s)
        nf = ch.process_device(x[a:b], b - a, chan_buf, s)
        nr = rs.process_device(chan_buf, nf, res_buf, s)
        picked = res_buf[:nr][:, cols].contiguous()
        got = wb.frames()
        assert got.shape == picked.shape, (a, b)
        assert torch.equal(torch.view_as_real(got).view(torch.int32), torch.view_as_real(picked).view(torch.int32)), (a, b)
        total += nr
        torch.cuda.synchronize()
    assert total == (cuts[-1] // D_SMALL * 18 + 24) // 25
    wb.close()
    ch.close()
    rs.close()


def _assert_known_answer(pkg, synth, got, cell, cells, tx, nslots):
    """test_rx.py::test_gpu_rx_all_kinds_cell_and_clock's assertions for each carrier j (channel j of the rows)."""
    R = pkg.rx_binding
    names = {R.KIND_SB1: "sb1", R.KIND_BBK: "bbk", R.KIND_SB2: "sb2", R.KIND_NDB1: "ndb1", R.KIND_NDB2: "ndb2", R.KIND_SCH_F: "schf"}
    by_time = {}
    for s in range(nslots):
        tn, fn, mn = synth.tdma_time_of_slot(s)
        by_time[tn | fn << 8 | mn << 16] = s
    for c, k in enumerate(BINS_SMALL):
        assert (cell[c].mcc, cell[c].mnc, cell[c].colour_code) == cells[k], (c, k)
        assert cell[c].scramb_init == synth.tx_scramb_code(*cells[k])
        exact = 0
        first = min(r[1] for r in got[R.KIND_SB1] if r[0] == c and r[2])
        for kind, name in names.items():
            sent = {s: v.tobytes() for s, v in tx[k][1][name]}
            rows = [r for r in got[kind] if r[0] == c and r[1] > first]
            assert len(rows) >= {"sb1": 8, "sb2": 8, "ndb1": 8, "ndb2": 8, "schf": 20, "bbk": 50}[name], (c, name, len(rows))
            for ch, bitnum, ok, t_rx, t, bits in rows:
                if bitnum < 28 * 510:
                    if ok and name != "bbk":
                        assert bits in sent.values(), (c, name, bitnum)
                    continue
                assert ok == 1 and t in by_time, (c, name, bitnum, hex(t))
                assert sent[by_time[t]] == bits, (c, name, by_time[t])
                exact += 1
        assert exact >= 5 * (nslots - 32) // 2, (c, exact)


def _run_collect(pkg, wb, xin, cuts):
    """Feed the cuts; rows of every call concatenated, without frame_slot (it counts frames per call), in (channel, bit number) order
    (a call returns its rows in (channel, frame) order)."""
    R = pkg.rx_binding
    got = {k: [] for k in range(R.N_KINDS)}
    for a, b in zip(cuts, cuts[1:]):
        wb.process_device(xin[a:b], b - a)
        for k, rows in _rows(wb.rx, R).items():
            got[k] += rows
    return {k: sorted(rows) for k, rows in got.items()}


@pytest.mark.gpu
def test_gpu_wbrx_known_answer_and_chunking(pkg, synth, small_capture):
    """After lock every carrier's cell state reads its (MCC, MNC, colour code); from slot 28 on its blocks come back with good CRCs
    and the type-1 bits of the slot their TDMA time names.  One call and ragged calls (some shorter than D) give the same rows."""
    import torch
    x, cells, tx = small_capture
    L = x.shape[0]
    one = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=L)
    got_one = _run_collect(pkg, one, x, [0, L])
    _assert_known_answer(pkg, synth, got_one, one.rx.cells(), cells, tx, 80)
    rng = np.random.default_rng(3)
    cuts = [0]
    while cuts[-1] < L:
        cuts.append(min(L, cuts[-1] + int(rng.choice([3, 15, 16, 17, 1000, 77777, 123456]))))
    many = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=123456)
    got_many = _run_collect(pkg, many, x, cuts)
    assert got_many == got_one
    assert [bytes(c) for c in many.rx.cells()] == [bytes(c) for c in one.rx.cells()]
    one.close()
    many.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_wbrx_full_size_cs16(pkg, synth):
    """20 MHz cs16 capture on the default config (M 800, FFT channeliser), carriers on bins 3 and 797 (a negative frequency) and two
    more: every carrier locks and reads its cell."""
    import torch
    bins = [797, 3, 555, 251]
    carriers = {797: 21, 3: 22, 555: 23, 251: 24}
    x, cells, tx = _capture(torch, synth, 800, carriers, 40)
    xs = _cs16(torch, x)
    del x
    L = xs.shape[0]
    wb = pkg.WidebandRx(bins, max_in=1 << 21)
    for a in range(0, L, 1 << 21):
        wb.process_device(xs[a:a + (1 << 21)])
    cell = wb.rx.cells()
    states = wb.rx.sync_states()
    for j, k in enumerate(bins):
        assert states[j][0] == pkg.bsync_binding.RX_S_LOCKED, (j, k)
        assert (cell[j].mcc, cell[j].mnc, cell[j].colour_code) == cells[k], (j, k)
    wb.close()


@pytest.mark.gpu
def test_gpu_wbrx_statuses_and_reset(pkg, small_capture):
    import torch
    R = pkg.rx_binding
    L = pkg.wbrx_binding._lib()
    for bad in ([], [-1], [32], [3, 5, 3], list(range(33))):
        with pytest.raises(pkg.TetraDemodError) as e:
            pkg.WidebandRx(bad, n_channels=32, decimation=16)
        assert e.value.status == ERR_ARG, bad
    x, _, _ = small_capture
    xs = _cs16(torch, x[:300000])
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=32, decimation=16, max_in=300000)
    assert wb.rx.count(R.KIND_SB1, 0) == 0 and wb.frames_device(1) == (None, 0)
    with pytest.raises(pkg.TetraDemodError) as e:
        wb.stage_ms()
    assert e.value.status == ERR_ARG
    big = torch.zeros(300001, dtype=torch.complex64, device="cuda")
    assert L.tetra_wbrx_process_device(wb._h, C.c_void_p(big.data_ptr()), 300001, None) == ERR_SIZE
    raw = torch.zeros(4 * 1000 + 16, dtype=torch.uint8, device="cuda")
    assert L.tetra_wbrx_process_device_cs16(wb._h, C.c_void_p(raw.data_ptr() + 2), 1000, None) == ERR_ALIGN
    assert L.tetra_wbrx_process_device(wb._h, C.c_void_p(raw.data_ptr() + 4), 1000, None) == ERR_ALIGN
    wb.process_device(xs)
    assert wb.rx.count(R.KIND_SB1, 1) == 0 and wb.frames_device(1)[1] == 0 and wb.frames_device(0)[1] > 0
    first = _rows(wb.rx, R)
    with pytest.raises(TypeError):
        wb.rx.reset()
    # reset: fresh receivers, the same output as a new handle
    wb.process_device(xs)
    wb.reset()
    assert wb.rx.count(R.KIND_SB1, 0) == 0 and all(c.scramb_init == 0 for c in wb.rx.cells())
    wb.process(xs.cpu().numpy())                       # the host path, cs16
    assert _rows(wb.rx, R) == first
    wb.close()


@pytest.mark.gpu
def test_gpu_wbrx_bin_power(pkg, small_capture):
    """Within 1e-5 relative of a float64 reduction of the full channeliser output of the same call; carriers stand out."""
    import torch
    x, _, _ = small_capture
    x = x[:400000]
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=32, decimation=16, max_in=400000)
    assert not wb.bin_power().any()
    ch = pkg.Channeliser(32, decimation=16, max_in=400000)
    for part in (x[:7], x[7:400000]):                  # the first call has no frame: zeros
        wb.process_device(part)
        buf = torch.zeros((max(1, (15 + part.shape[0]) // 16), 32), dtype=torch.complex64, device="cuda")
        nf = ch.process_device(part, part.shape[0], buf)
        got = wb.bin_power()
        if nf == 0:
            assert not got.any()
            continue
        want = (buf[:nf].to(torch.complex128).abs() ** 2).mean(0).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-5 * want.max(), np.abs(got / want - 1).max()
        assert np.all(np.abs(got / want - 1) <= 1e-5)
        noise = np.delete(got, BINS_SMALL + [0, 2, 6, 8, 19, 21, 30])
        assert got[BINS_SMALL].min() > 100 * noise.max()
    wb.close()


@pytest.mark.gpu
def test_gpu_wbrx_destroyed_handles_give_their_memory_back(pkg, small_capture):
    import torch
    x, _, _ = small_capture
    xs = _cs16(torch, x[:200000])

    def cycle():
        wb = pkg.WidebandRx(BINS_SMALL, n_channels=32, decimation=16, max_in=200000)
        wb.process_device(xs)
        wb.process(xs.cpu().numpy())
        wb.bin_power()
        wb.rx.fetch(pkg.rx_binding.KIND_SCH_F)
        wb.rx.deliver().wait()
        wb.close()
        full = pkg.WidebandRx(list(range(32)), n_channels=32, decimation=16, max_in=200000)
        full.process_device(xs)
        full.close()
        torch.cuda.synchronize()

    cycle()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        cycle()
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
