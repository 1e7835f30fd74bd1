"""What the wideband front end's stages share (channeliser, resampler): the window design (csrc/chan_design.hpp), the modulated
taps in their two layouts (csrc/chan_fft_core.hpp), and the delay line with its carry rule (DelayLine, csrc/hip_host.hpp) -- on the
host against the oracle and a numpy definition, on the GPU through each of the delay line's three users."""
import numpy as np
import pytest

from tests.test_chan_shift import ODD_LARGE, TWO32, ShiftedBankDefinition, _hc, _noise, _quantise

# ---------------------------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("M,P", [(800, 8), (32, 4), (2, 1), (4096, 2)])
def test_window_design_is_the_channeliser_oracles(oracle, M, P):
    """chandesign::kaiser_sinc compiled on its own, with the arguments tetra_chan.hip's design_prototype passes (beta 9, unity gain,
    fc = cutoff_rel / 2M), equals oracle/chan_oracle.c's restatement bit for bit."""
    from tests.emul import chan_design_shim_bind as cd
    assert np.array_equal(cd.kaiser_sinc(M * P, 1.2 / (2.0 * M), 9.0, 1.0), oracle.ChanOracle(M, P, M).h)


@pytest.mark.parametrize("I,DN,T,beta", [(18, 25, 16, 6.0), (1, 1, 2, 6.0), (4096, 4095, 2, 6.0), (7, 3, 64, 6.0), (18, 25, 16, 0.0)])
def test_window_design_is_the_resampler_oracles(oracle, I, DN, T, beta):
    """The same with tetra_resamp.hip's arguments: gain I, fc = cutoff_rel / 2 max(I, DN); beta 6 and the rectangular window."""
    from tests.emul import chan_design_shim_bind as cd
    want = oracle.ResampOracle(1, I, DN, T, beta=beta).h
    assert np.array_equal(cd.kaiser_sinc(I * T, 1.0 / (2.0 * max(I, DN)), beta, float(I)), want)


@pytest.mark.parametrize("P", [4, 6, 8])
@pytest.mark.parametrize("inc", [1, TWO32 // 1600, ODD_LARGE])
def test_tap_layouts_agree(oracle, P, inc):
    """tetra_chan_set_shift's two layouts of the modulated taps come from one modulated_tap: the fold layout [800][2][P] holds the
    [L] taps under its index map (parity 0: l = u + 800 q, parity 1: l = (u + 400) mod 800 + 800 q) bit for bit, and the [L] taps are
    the definition's hc to float32 rounding."""
    from tests.emul import chan_emul_bind as ce
    h = oracle.ChanOracle(800, P, 400).h
    lin, fold = ce.shift_taps(P, h, inc)
    u, q = np.arange(800)[:, None], np.arange(P)[None, :]
    assert np.array_equal(fold[:, 0, :].view(np.uint32), lin[u + 800 * q].view(np.uint32))
    assert np.array_equal(fold[:, 1, :].view(np.uint32), lin[(u + 400) % 800 + 800 * q].view(np.uint32))
    assert np.abs(lin - _hc(h, inc)).max() <= 2.0 ** -24 * np.abs(h).max()


def carry_rule(line, new):
    """DelayLine::carry written out: the other buffer takes keep = rows - min(n_in, rows) rows of the old line from row n_in on, then
    the from_x = min(n_in, rows) newest input rows; an empty call leaves the line alone."""
    rows, n_in = len(line), len(new)
    if n_in == 0:
        return line
    from_x = min(n_in, rows)
    keep = rows - from_x
    other = np.empty_like(line)
    other[:keep] = line[n_in:n_in + keep]
    other[keep:] = new[n_in - from_x:]
    return other


def test_carry_rule_keeps_the_newest_rows():
    """The rule against what it stands for, the last `rows` of [delay line | new]: rows = 7, calls shorter than, as long as and
    longer than the line, and an empty one."""
    rng = np.random.default_rng(7)
    line = rng.standard_normal((7, 3))
    for n in (0, 1, 6, 7, 8, 60):
        new = rng.standard_normal((n, 3))
        got = carry_rule(line, new)
        assert np.array_equal(got, np.concatenate([line, new])[-7:]), n
        line = got


CHAN_CALLS = [0, 1, 399, 3198, 3199, 3200, 7000]       # L - 1 = 3199 samples of delay line at P = 4
RESAMP_CALLS = [0, 1, 6, 7, 8, 60]                      # T - 1 = 7 frames at T = 8


def test_carry_rule_through_the_channeliser_emulation(oracle):
    """The merged channeliser emulation's carried state follows the rule over the three regimes (n_in = 0, 0 < n_in < L - 1, n_in >=
    L - 1), un-shifted and shifted, and with it the ragged stream gives the frames of one call, bit for bit."""
    from tests.emul import chan_emul_bind as ce
    h = oracle.ChanOracle(800, 4, 400).h
    x = _noise(np.random.default_rng(5), sum(CHAN_CALLS))
    for inc in (0, TWO32 // 1600):
        em, line, at, parts = ce.ChanFftShiftEmul(4, h, inc), np.zeros(3199, np.complex64), 0, []
        for n in CHAN_CALLS:
            parts.append(em.process(x[at:at + n]))
            line = carry_rule(line, x[at:at + n])
            at += n
            assert np.array_equal(em.hist, line), n
        whole = ce.ChanFftShiftEmul(4, h, inc).process(x)
        assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32)), inc


@pytest.mark.parametrize("cols", [None, [3, 0]])
def test_carry_rule_through_the_resampler_emulation(oracle, cols):
    from tests.emul import resamp_emul_bind as re_
    proto = oracle.ResampOracle(4, 18, 25, 8).h
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((sum(RESAMP_CALLS), 4)) + 1j * rng.standard_normal((sum(RESAMP_CALLS), 4))).astype(np.complex64)
    kept = x if cols is None else x[:, cols]
    em, line, at, parts = re_.ResampEmul(4, 18, 25, 8, proto, cols=cols), np.zeros((7, kept.shape[1]), np.complex64), 0, []
    for n in RESAMP_CALLS:
        parts.append(em.process(x[at:at + n]))
        line = carry_rule(line, kept[at:at + n])
        at += n
        assert np.array_equal(em.hist, line), n
    whole = re_.ResampEmul(4, 18, 25, 8, proto, cols=cols).process(x)
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------- GPU


def _chan_carry(pkg, M, P, D, calls, dtype, inc, flags=0):
    """One handle over calls of these lengths against the definition; -> the worst error relative to the call's largest output."""
    x = _noise(np.random.default_rng(M + P), sum(calls))
    raw, val = (x, x) if dtype == np.complex64 else _quantise(x.astype(np.complex128), dtype)
    ch = pkg.Channeliser(M, P, D, max_in=max(calls), flags=flags, shift=inc)
    d = ShiftedBankDefinition(M, P, D, ch.prototype(), inc)
    at, worst, frames = 0, 0.0, 0
    for n in calls:
        assert ch.frames_for(n) == (at % D + n) // D
        yg, yd = _chan_process(ch, raw[at:at + n], M), d.process(val[at:at + n])
        at += n
        assert yg.shape == yd.shape, n
        if len(yd):
            worst = max(worst, np.abs(yg - yd).max() / np.abs(yd).max())
            frames += len(yd)
    ch.close()
    assert frames == sum(calls) // D
    return worst


def _chan_process(ch, x, M):
    """Channeliser.process for complex64 input; the integer formats go through process_device."""
    if x.dtype == np.complex64:
        return ch.process(x)
    import torch
    out = torch.zeros((max(1, ch.frames_for(len(x))), M), dtype=torch.complex64, device="cuda")
    n = ch.process_device(torch.from_numpy(np.ascontiguousarray(x)).to("cuda") if len(x) else torch.zeros((1, 2), dtype=torch.int16, device="cuda"), len(x), out)
    torch.cuda.synchronize()
    return out[:n].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.complex64, np.int16])
@pytest.mark.parametrize("inc", [0, TWO32 // 1600])
def test_gpu_carry_regimes_fft_route(pkg, oracle, dtype, inc):
    """The delay line's three regimes through the FFT route (M 800, P 4, D 400: new samples read in place, carried with a copy or a
    format conversion): calls of 0, 1, 399 (shorter than the line of 3199), 3198, 3199, 3200 and 7000 samples on one handle, complex64
    and int16, un-shifted and with half a bin of shift, against the definition within test_chan.py's and test_chan_shift.py's 2e-5 of
    the call's largest output.  test_chan_shift.py::test_gpu_shifted_matches_definition[800-4-400-16401-0] runs 0 < n_in < rows and
    n_in >= rows for complex64 on this geometry; it has no empty call and none of exactly rows - 1, rows and rows + 1 samples, and a
    stream cannot leave a call out, so all seven stay."""
    err = _chan_carry(pkg, 800, 4, 400, CHAN_CALLS, dtype, inc)
    print("carry_fft_route_error %s inc %d: %.3e" % (np.dtype(dtype).name, inc, err))
    assert err < 2e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("inc", [0, TWO32 // 64])
def test_gpu_carry_regimes_staged_route(pkg, oracle, inc):
    """The same through the staged route (M 32, P 4, D 16: [line | new] in one buffer, one copy): calls of 0, 1, 15, 126, 127 (the
    line), 128 and 500 samples."""
    err = _chan_carry(pkg, 32, 4, 16, [0, 1, 15, 126, 127, 128, 500], np.complex64, inc)
    print("carry_staged_route_error inc %d: %.3e" % (inc, err))
    assert err < 2e-5, err


@pytest.mark.gpu
def test_gpu_carry_regimes_resampler(pkg, oracle):
    """And through the resampler (C 4, 18 / 25, T 8: a line of 7 frames): calls of 0, 1, 6, 7, 8 and 60 frames against the definition
    within test_resamp.py's tolerance.  (The picked-column carry runs in test_wbrx.py's ragged calls.)"""
    from tests.test_resamp import TOL
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((sum(RESAMP_CALLS), 4)) + 1j * rng.standard_normal((sum(RESAMP_CALLS), 4))).astype(np.complex64)
    rs, ro = pkg.Resampler(4, 18, 25, 8, max_in=max(RESAMP_CALLS)), oracle.ResampOracle(4, 18, 25, 8)
    at, worst, total = 0, 0.0, 0
    for n in RESAMP_CALLS:
        assert rs.frames_for(n) == ro.frames_for(n)
        yg, yo = rs.process(x[at:at + n]), ro.process(x[at:at + n])
        at += n
        assert yg.shape == yo.shape, n
        if len(yo):
            worst = max(worst, np.abs(yg - yo).max() / np.abs(yo).max())
            total += len(yo)
    rs.close()
    print("carry_resampler_error: %.3e" % worst)
    assert total == (sum(RESAMP_CALLS) * 18 + 24) // 25 and worst < TOL, worst
