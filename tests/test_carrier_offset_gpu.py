"""Per-carrier frequency offsets of the wideband receiver (include/ext/tetra_carrier_offset.h) on the GPU: the mixing kernels against the
double-precision definition applied to the channeliser's own output; zero offsets against a handle that never heard of them, bit for
bit; carriers a quarter of a bin off their centres decoded to the known answer (and to nothing without the offsets); retunes that keep
and change offsets; ordering across streams, the getter, reset.

Test band: tests/test_wbrx.py's small one (M 32, D 16, four carriers, 80 slots), built like its _capture with carrier k at
(k + e_k) / M cycles per sample."""
import math

import numpy as np
import pytest

from tests.chain_gpu import bit_rows as _bit_rows
from tests.test_carrier_offset import ODD_LARGE, TOL, definition
from tests.test_wbrx import BINS_SMALL, CARRIERS_SMALL, D_SMALL, M_SMALL, _assert_known_answer, _rows, _run_collect

NSLOTS = 80
FS = M_SMALL * 25000.0
OFF_HZ = [0.0, 6250.0, -6250.0, 0.0]                  # the carriers' own offsets from their bins' centres, slot by slot
# The channeliser prototype that has room for them: the cutoff in the middle between the carrier's far edge and the
# nearest edge of what aliases onto it, which is the bin spacing itself whatever the offset.
CHAN_CUTOFF_REL, CHAN_TAPS = 2.0, 16
ORACLE_SCHF_GOOD = {1: 30, 2: 33}                     # CRC-good SCH/F blocks of the oracle composition on the off-centre slots


def _capture_offsets(torch, synth, M, carriers, nslots, off_hz, seed=1, noise=1e-3):
    """tests/test_wbrx.py::_capture with carrier k at (k + e_k) Fs / M, e_k = off_hz[k] / 25 kHz."""
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
        x += y * torch.polar(torch.ones_like(n), 2.0 * math.pi * (kc + off_hz[k] / 25000.0) / M * n)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x += noise * torch.view_as_complex(torch.randn((L, 2), device=dev, generator=g, dtype=torch.float64))
    x *= 0.25 / float(x.abs().max())
    return x.to(torch.complex64).contiguous(), cells, tx


@pytest.fixture(scope="module")
def band(pkg, synth):
    import torch
    return _capture_offsets(torch, synth, M_SMALL, CARRIERS_SMALL, NSLOTS, dict(zip(BINS_SMALL, OFF_HZ)))


def _inc(pkg, hz):
    return pkg.wbrx_binding.carrier_offset_from_hz(hz, FS, D_SMALL)


def _u32(torch, t):
    return torch.view_as_real(t).view(torch.int32)


def _chan_frames(pkg, torch, x, cuts, max_in, **kw):
    """The Channeliser's frames of the same capture and cuts, [frames][M] complex64 on the host."""
    ch = pkg.Channeliser(M_SMALL, decimation=D_SMALL, max_in=max_in, **kw)
    buf = torch.zeros(((D_SMALL - 1 + max_in) // D_SMALL, M_SMALL), dtype=torch.complex64, device="cuda")
    out = []
    for a, b in zip(cuts, cuts[1:]):
        nf = ch.process_device(x[a:b], b - a, buf)
        out.append(buf[:nf].cpu().numpy().copy())
    ch.close()
    return np.concatenate(out)


# T = 10 has no specialised kernel (resamp_core.hpp's table): the generic one runs.  shift: the channeliser's common shift (a third of a
# bin) under the offsets -- the two compose, the definition being applied to the SHIFTED Channeliser's output.
@pytest.mark.gpu
@pytest.mark.parametrize("T,shift", [(8, 0), (16, 0), (24, 0), (10, 0), (16, (1 << 32) // (3 * M_SMALL))])
def test_gpu_mixed_frames_meet_the_definition(pkg, band, T, shift):
    """tetra_wbrx_frames_device with offsets {0, +inc_a, -inc_b, an odd large one} on the four slots against the float64 definition
    applied to the Channeliser's output of the same capture: within 2e-5 of the output's maximum.  The cuts hold an empty call, a
    5-sample call (no frame), calls that bring fewer frames than the delay line holds, and calls of many groups."""
    import torch
    x = band[0][:60000]
    cuts = [0, 0, 5, 5 + 9, 5 + 9 + 16 * (T - 3), 3001, 3001 + 37, 30011, 60000]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    inc = [0, _inc(pkg, 6250.0), _inc(pkg, -3125.0), ODD_LARGE]
    wb = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in, taps_per_phase=T, shift=shift)
    wb.set_offsets(inc)
    assert list(wb.offsets()) == inc and wb.get_shift() == shift
    got = []
    for a, b in zip(cuts, cuts[1:]):
        wb.process_device(x[a:b], b - a)
        got.append(wb.frames().cpu().numpy().copy())
    got = np.concatenate(got)
    rs = pkg.Resampler(4, taps_per_phase=T, max_in=16)
    h = rs.prototype()
    rs.close()
    f = _chan_frames(pkg, torch, x, cuts, max_in, shift=shift)
    want = definition(f, 0, BINS_SMALL, inc, h, 18, 25, T, 0, got.shape[0])
    assert got.shape == want.shape and got.shape[0] == (f.shape[0] * 18 + 24) // 25
    err = np.abs(got - want).max() / np.abs(want).max()
    print("carrier offset, GPU frames vs definition, T %d, shift %d: worst %.3g of the maximum" % (T, shift, err))
    assert err <= TOL, err
    plain = definition(f, 0, BINS_SMALL, [0, 0, 0, 0], h, 18, 25, T, 0, got.shape[0])
    assert np.abs(got[:, 0] - plain[:, 0]).max() <= TOL * np.abs(want).max()          # the slot at 0 among them: un-rotated
    assert np.abs(got[:, 1] - plain[:, 1]).max() > 0.1 * np.abs(want).max()           # (and the others are not)
    wb.close()


@pytest.mark.gpu
def test_gpu_zero_offsets_change_nothing(pkg, band):
    """A handle on which the setter was called with all zeros (before the first call and between calls) against a handle that never
    called it: frames, every kind's rows, bit rows, cells and sync states are equal, bit for bit, call for call."""
    import torch
    R = pkg.rx_binding
    x = band[0]
    L = x.shape[0]
    cuts = [0, 5, 5 + 9, 200003, 200003 + 16 * 1000 + 7, 470000, 470010, L]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    a_ = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in)
    b_ = pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in, offsets_hz=[0.0] * 4)
    s = torch.cuda.current_stream()
    for lo, hi in zip(cuts, cuts[1:]):
        b_.set_offsets([0, 0, 0, 0], stream=s)
        a_.process_device(x[lo:hi], hi - lo, s)
        b_.process_device(x[lo:hi], hi - lo, s)
        assert torch.equal(_u32(torch, a_.frames()), _u32(torch, b_.frames())), (lo, hi)
        assert _rows(a_.rx, R) == _rows(b_.rx, R), (lo, hi)
        assert _bit_rows(torch, a_.rx, 4) == _bit_rows(torch, b_.rx, 4), (lo, hi)
        torch.cuda.synchronize()
    assert [bytes(c) for c in a_.rx.cells()] == [bytes(c) for c in b_.rx.cells()]
    assert a_.rx.sync_states() == b_.rx.sync_states()
    assert not b_.offsets().any() and not a_.offsets().any()
    a_.close()
    b_.close()


def _schf_good(pkg, got, c):
    return len([r for r in got[pkg.rx_binding.KIND_SCH_F] if r[0] == c and r[2]])


@pytest.mark.gpu
def test_gpu_off_centre_carriers_known_answer(pkg, synth, band):
    """Carriers 1 and 31 on their bins' centres, carrier 7 at +6.25 kHz and carrier 20 at -6.25 kHz (a quarter of a bin), channeliser
    prototype chan_cutoff_rel 2.0, taps_per_channel 16.  The oracle composition (profiles/carrier_offset_composition.py: channeliser
    oracle -> numpy pre-mix -> resampler oracle -> oracle demodulator -> the reference's chain in oracle/_ref) on the same band with
    these values decodes 30 (+6.25 kHz) and 33 (-6.25 kHz) CRC-good SCH/F blocks on the off-centre carriers, 33 and 35 on the centred
    ones, no CRC-bad one behind the eighth, and none at all on the off-centre carriers without the pre-mix.  (taps_per_channel 8 gives
    25 and 33 there, every SCH/F block CRC-good too, but on the GPU one AACH bit of one block of carrier 7 is then wrong from 4.7 kHz
    on: DESIGN.md 8.12.)

    With the offsets set every carrier passes tests/test_wbrx.py's known-answer assertions and the off-centre ones deliver at least
    those counts; with the offsets left at zero the off-centre carriers deliver no CRC-good SCH/F block while the centred ones decode
    as before."""
    import torch
    R = pkg.rx_binding
    x, cells, tx = band
    L = x.shape[0]
    kw = dict(n_channels=M_SMALL, decimation=D_SMALL, max_in=L, chan_cutoff_rel=CHAN_CUTOFF_REL, taps_per_channel=CHAN_TAPS)
    on = pkg.WidebandRx(BINS_SMALL, offsets_hz=OFF_HZ, **kw)
    assert list(on.offsets()) == [0, 1 << 29, (1 << 32) - (1 << 29), 0]
    got = _run_collect(pkg, on, x, [0, L])
    _assert_known_answer(pkg, synth, got, on.rx.cells(), cells, tx, NSLOTS)
    for c, want in ORACLE_SCHF_GOOD.items():
        n = _schf_good(pkg, got, c)
        print("slot %d (%+.0f Hz): %d CRC-good SCH/F blocks (oracle composition: %d)" % (c, OFF_HZ[c], n, want))
        assert n >= want, (c, n, want)
    on.close()
    off = pkg.WidebandRx(BINS_SMALL, **kw)
    got0 = _run_collect(pkg, off, x, [0, L])
    cell = off.rx.cells()
    for c in (1, 2):
        assert _schf_good(pkg, got0, c) == 0, c
    for c in (0, 3):
        assert (cell[c].mcc, cell[c].mnc, cell[c].colour_code) == cells[BINS_SMALL[c]], c
        rows = [r for r in got0[R.KIND_SCH_F] if r[0] == c]
        assert _schf_good(pkg, got0, c) >= 20 and all(r[2] == 1 for r in rows if r[1] >= 28 * 510), c
        assert [r for r in rows if r[2]] == [r for r in got[R.KIND_SCH_F] if r[0] == c and r[2]], c      # the mixer next door changes nothing here
    off.close()
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_retune_keeps_and_changes_offsets(pkg, band):
    """Before call 3 slot 1 moves from bin 7 to bin 12 and keeps its offset; slot 2 moves from bin 20 to bin 25 and gets a new offset in
    the same gap (retune(bins, offsets=...)).  From that call on the moved slots' frames are those of a fresh handle on the new bins and
    offsets fed the same capture from the start, first frame included (within 2e-5 of the maximum: the delay line is rebuilt from
    un-rotated frames and the phase is the absolute frame's); slots 0 and 3 stay bit-identical to a handle that was never retuned."""
    import torch
    x = band[0][:120000]
    cuts = [0, 7, 7 + 16 * 9, 20000, 20000 + 5, 60011, 120000]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    old = [0, _inc(pkg, 6250.0), _inc(pkg, -6250.0), ODD_LARGE]
    new_bins, new = [1, 12, 25, 31], [0, old[1], _inc(pkg, 1562.5), ODD_LARGE]
    kw = dict(n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in)
    moved = pkg.WidebandRx(BINS_SMALL, **kw)
    never = pkg.WidebandRx(BINS_SMALL, **kw)
    fresh = pkg.WidebandRx(new_bins, **kw)
    moved.set_offsets(old)
    never.set_offsets(old)
    fresh.set_offsets(new)
    worst = 0.0
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        if k == 3:
            moved.retune(new_bins, offsets=new)
            assert list(moved.offsets()) == new and list(moved.bins()) == new_bins
        for wb in (moved, never, fresh):
            wb.process_device(x[lo:hi], hi - lo)
        fm, fn, ff = moved.frames(), never.frames(), fresh.frames()
        assert fm.shape == fn.shape == ff.shape
        assert torch.equal(_u32(torch, fm[:, [0, 3]].contiguous()), _u32(torch, fn[:, [0, 3]].contiguous())), k
        if fm.shape[0] == 0:
            continue
        if k < 3:
            assert torch.equal(_u32(torch, fm), _u32(torch, fn)), k
        else:
            scale = float(ff.abs().max())
            err = float((fm[:, 1:3] - ff[:, 1:3]).abs().max()) / scale
            worst = max(worst, err)
            assert err <= TOL, (k, err)
            assert float((fm[:, 1:3] - fn[:, 1:3]).abs().max()) > 0.1 * scale, k
        torch.cuda.synchronize()
    print("retuned slots vs a fresh handle on the new bins and offsets: worst %.3g of the maximum" % worst)
    for wb in (moved, never, fresh):
        wb.close()


@pytest.mark.gpu
def test_gpu_offsets_across_streams_getter_reset_and_full_width(pkg, band):
    """A setter call on another stream than the process call before it, with no wait anywhere, is ordered behind that call and ahead of
    the next: every call's frames equal the single-stream run's, bit for bit.  get returns what was set; an equal list is accepted;
    offsets survive tetra_wbrx_reset and the stream after it equals a fresh handle's.  A full-width handle (bins 0 .. M - 1, the in-place
    resampler) takes offsets too and then gives, on the carriers' bins, the picked handle's frames."""
    import torch
    x = band[0][:160000]
    cuts = [0, 40000, 80003, 120000, 160000]
    plan = {0: [0, 5, 6, 7], 1: [ODD_LARGE, 1, 0, _inc(pkg, 6250.0)], 2: [0, 0, 0, 0], 3: [1 << 31, 0, 3, 0]}
    kw = dict(n_channels=M_SMALL, decimation=D_SMALL, max_in=40003)
    one = pkg.WidebandRx(BINS_SMALL, **kw)
    two = pkg.WidebandRx(BINS_SMALL, **kw)
    s0 = torch.cuda.current_stream()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(s0)
    sb.wait_stream(s0)
    want = []
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        one.set_offsets(plan[k], stream=s0)
        one.process_device(x[lo:hi], hi - lo, s0)
        want.append(one.frames(stream=s0).clone())
    torch.cuda.synchronize()
    got = []
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        s_set, s_run = (sa, sb) if k % 2 == 0 else (sb, sa)
        two.set_offsets(plan[k], stream=s_set)
        assert list(two.offsets()) == plan[k]
        two.process_device(x[lo:hi], hi - lo, s_run)
        with torch.cuda.stream(s_run):
            got.append(two.frames(stream=s_run).clone())
    torch.cuda.synchronize()
    for k in range(len(want)):
        assert torch.equal(_u32(torch, want[k]), _u32(torch, got[k])), k
    two.set_offsets(plan[3])                      # the list in force: nothing to do
    # reset keeps the offsets and restarts the frame count
    two.reset()
    assert list(two.offsets()) == plan[3]
    fresh = pkg.WidebandRx(BINS_SMALL, **kw)
    fresh.set_offsets(plan[3])
    two.process_device(x[:40000], 40000)
    fresh.process_device(x[:40000], 40000)
    assert torch.equal(_u32(torch, two.frames()), _u32(torch, fresh.frames()))
    # full width
    inc_all = [0] * M_SMALL
    for j, k in enumerate(BINS_SMALL):
        inc_all[k] = plan[3][j]
    full = pkg.WidebandRx(list(range(M_SMALL)), **kw)
    full.process_device(x[:7], 7)                 # (a call in place first)
    fresh.reset()
    fresh.process_device(x[:7], 7)
    full.set_offsets(inc_all)
    full.process_device(x[7:40000], 39993)
    fresh.process_device(x[7:40000], 39993)
    assert torch.equal(_u32(torch, full.frames()[:, BINS_SMALL].contiguous()), _u32(torch, fresh.frames()))
    assert list(full.offsets()) == inc_all
    for wb in (one, two, fresh, full):
        wb.close()
    torch.cuda.synchronize()
