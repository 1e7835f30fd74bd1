"""The wideband receiver on carriers that lie OFF the bins' centres (include/tetra_shift.h: tetra_wbrx_set_shift).

The capture is tests/test_wbrx.py's small one -- same geometry (32 bins at 800 kHz, D 16), same seeds, same coded downlinks from
synth.gen_downlink -- with every carrier placed at (k + 0.5) Fs / M instead of k Fs / M.  With half a bin of shift the receiver must
give the known answer the existing test asks of the on-grid capture; without the shift it must lock nothing."""
import math

import numpy as np
import pytest

from tests.test_wbrx import (BINS_SMALL, CARRIERS_SMALL, D_SMALL, M_SMALL, _assert_known_answer, _cs16, _rows, _run_collect)

HALF_BIN = (1 << 32) // (2 * M_SMALL)
NSLOTS = 80


def _capture_off_grid(torch, synth, M, carriers, nslots, offset_bins, seed=1, noise=1e-3):
    """tests/test_wbrx.py::_capture with every carrier at (k + offset_bins) Fs / M."""
    dev = torch.device("cuda")
    fs = M * 25000.0
    N = (nslots * 510 - 100) // 9 * 9
    L = int(round(N * fs / 36000.0))
    x = torch.zeros(L, dtype=torch.complex128, device=dev)
    n = torch.arange(L, dtype=torch.float64, device=dev)
    cells, tx = {}, {}
    for k, sd in carriers.items():
        cells[k] = (100 + 7 * sd % 900, 1000 + 13 * sd, (5 + 3 * sd) % 64)
        tx[k] = synth.gen_downlink(nslots, sd, cell=cells[k])
        s = torch.from_numpy(synth.gen_channel(N, sd + 100, bits=tx[k][0], amp=1.0)[0].astype(np.complex128)).to(dev)
        S = torch.fft.fft(s)
        Y = torch.zeros(L, dtype=torch.complex128, device=dev)
        Y[: N // 2] = S[: N // 2]
        Y[L - (N - N // 2):] = S[N // 2:]
        y = torch.fft.ifft(Y) * (L / N)
        kc = k if k < M // 2 else k - M
        x += y * torch.polar(torch.ones_like(n), 2.0 * math.pi * (kc + offset_bins) / M * n)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x += noise * torch.view_as_complex(torch.randn((L, 2), device=dev, generator=g, dtype=torch.float64))
    x *= 0.25 / float(x.abs().max())
    return x.to(torch.complex64).contiguous(), cells, tx


@pytest.fixture(scope="module")
def off_grid_capture(pkg, synth):
    import torch
    return _capture_off_grid(torch, synth, M_SMALL, CARRIERS_SMALL, NSLOTS, 0.5)


@pytest.mark.gpu
def test_gpu_wbrx_half_bin_shift_known_answer_and_chunking(pkg, synth, off_grid_capture):
    """(a) WidebandRx(bins, shift = half a bin) on the half-bin capture: every carrier's cell state reads its (MCC, MNC, colour code);
    from slot 28 on every block is CRC-good with the type-1 bits of the slot its TDMA time names (test_wbrx.py's own assertions);
    one call and ragged calls (some shorter than D) give identical rows -- the phase reference does not depend on the cuts."""
    import torch
    x, cells, tx = off_grid_capture
    L = x.shape[0]
    one = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=L, shift=HALF_BIN)
    assert one.get_shift() == HALF_BIN
    got_one = _run_collect(pkg, one, x, [0, L])
    _assert_known_answer(pkg, synth, got_one, one.rx.cells(), cells, tx, NSLOTS)
    rng = np.random.default_rng(3)
    cuts = [0]
    while cuts[-1] < L:
        cuts.append(min(L, cuts[-1] + int(rng.choice([3, 15, 16, 17, 1000, 77777, 123456]))))
    many = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=123456)
    many.set_shift(HALF_BIN)
    got_many = _run_collect(pkg, many, x, cuts)
    assert got_many == got_one
    assert [bytes(c) for c in many.rx.cells()] == [bytes(c) for c in one.rx.cells()]
    one.close()
    many.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_wbrx_without_the_shift_the_half_bin_capture_locks_nothing(pkg, off_grid_capture):
    """(b) The same capture with shift 0: the prototype cuts every carrier in half -- no CRC-good SB1 on any bin."""
    R = pkg.rx_binding
    x, _, _ = off_grid_capture
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=x.shape[0])
    assert wb.get_shift() == 0
    got = _run_collect(pkg, wb, x, [0, x.shape[0]])
    assert not [r for r in got[R.KIND_SB1] if r[2]]
    wb.close()


@pytest.mark.gpu
def test_gpu_wbrx_half_bin_shift_cs16_gives_the_rows_of_complex64_on_the_quantised_samples(pkg, off_grid_capture):
    """(c) cs16 in, against complex64 in on the same quantised samples (integer / 32768): identical rows and cell states."""
    import torch
    x, _, _ = off_grid_capture
    xs = _cs16(torch, x)
    xq = torch.view_as_complex((xs.to(torch.float32) / 32768.0).contiguous())
    L = x.shape[0]
    cuts = [0, 100003, 100003 + 7, 500000, L]
    a = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=L, shift=HALF_BIN)
    b = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=L, shift=HALF_BIN)
    got_a, got_b = _run_collect(pkg, a, xs, cuts), _run_collect(pkg, b, xq, cuts)
    assert got_a == got_b and len(got_a[pkg.rx_binding.KIND_SB1]) > 8
    assert [bytes(c) for c in a.rx.cells()] == [bytes(c) for c in b.rx.cells()]
    a.close()
    b.close()


@pytest.mark.gpu
def test_gpu_wbrx_bin_power_of_the_shifted_bins(pkg, off_grid_capture):
    """tetra_wbrx_bin_power under half a bin of shift: test_wbrx.py::test_gpu_wbrx_bin_power's comparison -- the listed bins against
    every bin neither listed nor next to a carrier, factor 100 -- and within its 1e-5 of a float64 reduction of the shifted
    channeliser's own output."""
    import torch
    x, _, _ = off_grid_capture
    x = x[:400000]
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=32, decimation=16, max_in=400000, shift=HALF_BIN)
    ch = pkg.Channeliser(32, decimation=16, max_in=400000, shift=HALF_BIN)
    for part in (x[:7], x[7:400000]):
        wb.process_device(part)
        buf = torch.zeros((max(1, (15 + part.shape[0]) // 16), 32), dtype=torch.complex64, device="cuda")
        nf = ch.process_device(part, part.shape[0], buf)
        got = wb.bin_power()
        if nf == 0:
            assert not got.any()
            continue
        want = (buf[:nf].to(torch.complex128).abs() ** 2).mean(0).cpu().numpy()
        assert np.abs(got - want).max() <= 1e-5 * want.max()
        assert np.all(np.abs(got / want - 1) <= 1e-5)
        noise = np.delete(got, BINS_SMALL + [0, 2, 6, 8, 19, 21, 30])
        assert got[BINS_SMALL].min() > 100 * noise.max()
    wb.close()
    ch.close()
