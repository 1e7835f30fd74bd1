"""The frequency-shifted channeliser (include/tetra_shift.h: tetra_chan_set_shift): carriers off the bins' centres by one common offset.

Expected values come from the DEFINITION, written out below in numpy complex128 (ShiftedBankDefinition): the un-shifted bank's sum
with the modulated prototype hc[l] = h[l] exp(+j 2 pi inc l / 2^32) and the frame phasor exp(-j 2 pi (inc n_m mod 2^32) / 2^32), both
phases in integer arithmetic -- cross-checked once against oracle.ChanOracle run on the premixed signal.  Against it: the FFT
kernel's shifted lane code on the host (tests/emul/chan_emul.cpp) and all three kernels on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_chan import SWEEP, _sweep_check, _sweep_cuts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
TWO32 = 1 << 32
ODD_LARGE = 0x9E3779B1          # an odd increment near 0.62 cycles per sample: inc * n wraps every other sample


def _hc(h, inc):
    """hc[l] = h[l] exp(+j 2 pi (inc l mod 2^32) / 2^32), complex128 from the float32 prototype."""
    l = np.arange(h.size, dtype=np.uint64)
    ph = ((l * np.uint64(inc)) & np.uint64(TWO32 - 1)).astype(np.float64) / TWO32
    return h.astype(np.float64) * np.exp(2j * np.pi * ph)


class ShiftedBankDefinition:
    """out'[m][k] = exp(-j 2 pi (inc n_m mod 2^32) / 2^32) . sum_l hc[l] x[n_m - l] exp(-j 2 pi k (n_m - l) / M), n_m = (m + 1) D - 1
    counted from the stream's first sample, x = 0 before it; complex128.  The sum over l is taken residue by residue of (n_m - l) mod M
    (P terms each) and the sum over the residues by np.fft: the same sum, re-associated."""

    def __init__(self, M, P, D, h, inc=0):
        self.M, self.P, self.D, self.L = M, P, D, M * P
        self.h = np.asarray(h, np.float32)
        self.buf = np.zeros(self.L - 1, np.complex128)      # buf[i] = x[i - (L - 1)]
        self.m = 0                                          # next frame
        self.set_shift(inc)

    def set_shift(self, inc):
        self.inc = int(inc) & (TWO32 - 1)
        self.hc = _hc(self.h, self.inc)

    def process(self, x):
        self.buf = np.concatenate([self.buf, np.asarray(x).astype(np.complex128)])
        n_have = self.buf.size - (self.L - 1)
        out = []
        M, P, L = self.M, self.P, self.L
        while (self.m + 1) * self.D <= n_have:
            n_m = (self.m + 1) * self.D - 1
            seg = self.buf[n_m + L - 1 - np.arange(L)]      # seg[l] = x[n_m - l]
            u = (self.hc * seg).reshape(P, M).sum(0)        # u[l0] = sum_q hc[l0 + q M] x[n_m - l0 - q M]
            v = np.zeros(M, np.complex128)
            v[(n_m - np.arange(M)) % M] = u                 # residue r = (n_m - l0) mod M
            ph = ((self.inc * n_m) % TWO32) / TWO32
            out.append(np.fft.fft(v) * np.exp(-2j * np.pi * ph))
            self.m += 1
        return np.array(out, np.complex128).reshape(-1, M)


def _quantise(x, dtype):
    full = 32768 if dtype == np.int16 else 128
    q = np.stack([np.clip(np.round(x.real * full / 6), -full, full - 1), np.clip(np.round(x.imag * full / 6), -full, full - 1)], axis=1).astype(dtype)
    return q, (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64) / np.float32(full)


def _noise(rng, n):
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


# ---------------------------------------------------------------------------------------------------------------------- CPU


def test_definition_is_the_unshifted_bank_on_the_premixed_signal(oracle):
    """The numpy definition against oracle.ChanOracle fed x[n] exp(-j 2 pi inc n / 2^32) premixed in complex128.  The oracle takes
    complex64 input, so the agreement is to the 1e-6 of the output's maximum that test_chan.py uses for the oracle, not bit for bit.
    inc = 0 is the un-shifted definition itself."""
    rng = np.random.default_rng(11)
    for M, P, D, inc in ((32, 4, 16, TWO32 // 64 + 12345), (32, 8, 16, 0), (800, 4, 400, TWO32 // 1600), (60, 4, 20, ODD_LARGE)):
        n = D * 25 + 3
        x = _noise(rng, n)
        d = ShiftedBankDefinition(M, P, D, oracle.ChanOracle(M, P, D).h, inc)
        got = np.concatenate([d.process(x[:n // 3]), d.process(x[n // 3:])])
        nn = np.arange(n, dtype=np.uint64)
        mix = np.exp(-2j * np.pi * ((nn * np.uint64(inc)) & np.uint64(TWO32 - 1)).astype(np.float64) / TWO32)
        want = oracle.ChanOracle(M, P, D).process((x.astype(np.complex128) * mix).astype(np.complex64))
        assert got.shape == want.shape
        assert np.abs(got - want).max() / np.abs(want).max() < 1e-6, (M, P, D, inc)


@pytest.mark.parametrize("P", [4, 6, 8])
@pytest.mark.parametrize("inc", [TWO32 // 1600, TWO32 // 3200, 1, TWO32 - 1, ODD_LARGE])
def test_shifted_lane_code_on_the_host_matches_the_definition(oracle, P, inc):
    """The SHIFT = true instantiations of csrc/chan_fft_core.hpp (complex fold, frame phasor in its LDS slot, store) thread by
    thread on the host against the definition: half a bin, a quarter bin, 1, 2^32 - 1 and an odd large increment (inc n_m wraps
    thousands of times within the stream: the integer phase must be exact), complex64 / int16 / int8 samples, ragged cuts with
    carried history, sub-frame phase and phase reference.  The emulation poisons all of LDS (pads too) before every block and
    the output rows, so an unwritten or overwritten phasor slot shows as NaN.  Bound 3e-6 of the output's maximum: the un-shifted
    lane code is held to 2e-6 (test_chan.py); the shifted one adds two roundings per tap (re and im of hc, 2^-24 each, P-term sums),
    one complex multiply per output (2^-23) and the phasor's 2^-24 phase quantum (1.9e-7 rad) -- under 1e-6 together."""
    from tests.emul import chan_emul_bind as cs
    rng = np.random.default_rng(100 * P + inc % 97)
    h = oracle.ChanOracle(800, P, 400).h
    nin = 400 * 19 + 123
    xf = _noise(rng, nin)
    q16, x16 = _quantise(xf.astype(np.complex128), np.int16)
    q8, x8 = _quantise(xf.astype(np.complex128), np.int8)
    cuts = [0, 7, 7 + 399, nin // 3, nin // 3 + 1, nin]
    for name, raw, val in (("c64", xf, xf), ("cs16", q16, x16), ("cs8", q8, x8)):
        em, em_f, d = cs.ChanFftShiftEmul(P, h, inc), cs.ChanFftShiftEmul(P, h, inc), ShiftedBankDefinition(800, P, 400, h, inc)
        for a, b in zip(cuts, cuts[1:]):
            ye, yd = em.process(raw[a:b]), d.process(val[a:b])
            assert ye.shape == yd.shape
            if name != "c64":            # the integer routes equal the complex64 route on the converted samples, bit for bit
                assert np.array_equal(ye.view(np.uint32), em_f.process(val[a:b]).view(np.uint32)), (name, a, b)
            if len(yd):
                assert np.isfinite(ye).all(), (name, a, b)
                err = np.abs(ye - yd).max() / np.abs(yd).max()
                assert err < 3e-6, (name, a, b, err)


def test_set_shift_mid_stream_on_the_host_keeps_the_phase_reference(oracle):
    from tests.emul import chan_emul_bind as cs
    rng = np.random.default_rng(8)
    h = oracle.ChanOracle(800, 8, 400).h
    x = _noise(rng, 400 * 30 + 77)
    em, d = cs.ChanFftShiftEmul(8, h, TWO32 // 1600), ShiftedBankDefinition(800, 8, 400, h, TWO32 // 1600)
    for i, (a, b) in enumerate(((0, 4001), (4001, 8100), (8100, x.size))):
        if i == 1:
            em.set_shift(ODD_LARGE), d.set_shift(ODD_LARGE)
        if i == 2:
            em.set_shift(0), d.set_shift(0)
        ye, yd = em.process(x[a:b]), d.process(x[a:b])
        assert ye.shape == yd.shape and np.abs(ye - yd).max() / np.abs(yd).max() < 3e-6, i


SHIFT_ZERO_NIN = 400 * 17 + 55
SHIFT_ZERO_CUTS = [0, 9, 9 + 399, SHIFT_ZERO_NIN // 2, SHIFT_ZERO_NIN]


def shift_zero_inputs(dtype):
    """(P, samples) of the shift-zero test, P = 4, 6, 8 off one generator (tests/golden/make_front_end_golden.py records from these)."""
    rng = np.random.default_rng(4)
    for P in (4, 6, 8):
        x = _noise(rng, SHIFT_ZERO_NIN)
        yield P, (x if dtype == np.complex64 else _quantise(x.astype(np.complex128), dtype)[0])


@pytest.mark.parametrize("dtype", [np.complex64, np.int16, np.int8])
def test_shift_zero_through_the_new_emulation_equals_the_existing_emulation(oracle, dtype):
    """inc = 0: the emulation's dispatch (un-shifted instantiations, as the library's) equals, bit for bit, the rows that
    tests/emul/chan_emul.cpp gave before the shifted emulation was folded into it (tests/golden/chan_emul_unshifted.npz: the first
    and last frame of every call; no libm call on this path); and the SHIFT = true lane code itself at inc = 0 (taps (h, 0), phasor
    (1, -0)) gives the same numbers (x . 1 - y . 0 is exact; only the sign of a zero can differ, hence array_equal on values)."""
    from tests.emul import chan_emul_bind as ce
    gold = np.load(os.path.join(ROOT, "tests", "golden", "chan_emul_unshifted.npz"))
    assert list(gold["cuts"]) == SHIFT_ZERO_CUTS
    for P, x in shift_zero_inputs(dtype):
        h = oracle.ChanOracle(800, P, 400).h
        plain, forced = ce.ChanFftShiftEmul(P, h, 0), ce.ChanFftShiftEmul(P, h, 0, force_shift_code=True)
        first = ce.ChanFftEmul(P, h)
        rows = []
        for a, b in zip(SHIFT_ZERO_CUTS, SHIFT_ZERO_CUTS[1:]):
            yn, yf = plain.process(x[a:b]), forced.process(x[a:b])
            assert np.array_equal(yn.view(np.uint32), first.process(x[a:b]).view(np.uint32)), (P, a, b)
            assert np.array_equal(yn, yf), (P, a, b)
            rows.append(yn)
        want = gold["%s_P%d" % (np.dtype(dtype).name, P)]
        assert np.array_equal(np.concatenate(rows)[gold["keep"]].view(np.uint32), want.view(np.uint32)), P


def test_host_phasor_is_the_integer_phase(oracle):
    from tests.emul import chan_emul_bind as cs
    for ph in (0, 1, TWO32 // 4, TWO32 // 2, TWO32 - 1, ODD_LARGE, 0x12345678):
        assert abs(cs.phasor(ph) - np.exp(-2j * np.pi * ph / TWO32)) < 3e-7, ph


def test_shift_header_symbols_all_exported(pkg):
    """Every entry point include/tetra_shift.h declares is exported and listed by the bindings; the pinned headers did not grow."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tetra_shift.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tetra_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(pkg.chan_binding.CHAN_SHIFT_EXPORTS + pkg.wbrx_binding.WBRX_SHIFT_EXPORTS) and len(names) == 5
    L = pkg.load_library()
    for n in names:
        assert hasattr(L, n), n


def test_shift_from_hz(pkg):
    f = pkg.chan_binding.shift_from_hz
    assert f(12500, 20e6) == round(TWO32 / 1600) == 2684355
    assert f(-12500, 20e6) == TWO32 - 2684355                 # negative shifts wrap
    assert f(0, 20e6) == 0 and f(20e6, 20e6) == 0 and f(10e6, 20e6) == TWO32 // 2
    assert f(6250, 800e3) == round(TWO32 / 128) and f(-6250, 800e3) == TWO32 - round(TWO32 / 128)
    assert f(12500, 0) == 0 and f(float("nan"), 20e6) == 0 and f(-1e-9, 20e6) == 0


def test_shift_entry_points_refuse_bad_handles(pkg):
    L = pkg.chan_binding._lib()
    pkg.wbrx_binding._lib()
    v = C.c_uint32(7)
    assert L.tetra_chan_set_shift(None, 5) == ERR_ARG and L.tetra_chan_get_shift(None, C.byref(v)) == ERR_ARG
    assert L.tetra_wbrx_set_shift(None, 5) == ERR_ARG and L.tetra_wbrx_get_shift(None, C.byref(v)) == ERR_ARG
    assert v.value == 7
    ch = pkg.Channeliser.__new__(pkg.Channeliser)             # a closed binding object: NULL handle
    ch._lib, ch._h = L, None
    with pytest.raises(pkg.TetraDemodError) as e:
        ch.set_shift(1)
    assert e.value.status == ERR_ARG
    with pytest.raises(pkg.TetraDemodError):
        ch.get_shift()
    wb = pkg.WidebandRx.__new__(pkg.WidebandRx)
    wb._lib, wb._h, wb.rx = L, None, None
    with pytest.raises(pkg.TetraDemodError) as e:
        wb.set_shift(1)
    assert e.value.status == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------- GPU

GEOMETRIES = [(32, 8, 16, 3000, 0), (800, 8, 400, 800 * 5, 0), (800, 8, 400, 800 * 5, 1), (800, 8, 400, 800 * 5, 2), (60, 4, 20, 1234, 0),
              (32, 4, 32, 1000, 0), (800, 8, 400, 400 * 1000 + 123, 0), (800, 8, 400, 400 * 120 + 7, 1),
              (800, 8, 400, 400 * 1000 + 123, 2), (800, 6, 400, 400 * 130 + 399, 0), (800, 4, 400, 400 * 41 + 1, 0),
              (800, 6, 800, 800 * 40, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,P,D,nin,flags", GEOMETRIES)
def test_gpu_shifted_matches_definition(pkg, oracle, M, P, D, nin, flags):
    """The geometries of test_chan.py::test_gpu_matches_definition (all three kernels) with half a bin of shift, ragged chunks, and
    a set_shift in the middle of the stream (to an odd large increment, at the fourth chunk): every chunk within 2e-5 of the
    output's maximum of the definition, the phase reference carried through.  Measured on MI355X over these cases (printed
    below as e0 / e1 per case), the un-shifted kernels' error e0 and the shifted kernels' e1 on the same inputs: e0 = 1.0e-7 .. 3.5e-7,
    e1 = 1.2e-7 .. 4.2e-7 (worst pair: matrix form, e0 2.5e-7, e1 4.2e-7; FFT form at 1000 frames: 1.4e-7, 1.8e-7).  e1 <= 2e-5, so
    the project's bound for this comparison is asserted as it stands."""
    rng = np.random.default_rng(M)
    x = _noise(rng, nin)
    half = TWO32 // (2 * M)
    ch = pkg.Channeliser(M, P, D, max_in=nin, flags=flags, shift=half)
    ch0 = pkg.Channeliser(M, P, D, max_in=nin, flags=flags)
    assert ch.get_shift() == half and ch0.get_shift() == 0
    h = ch.prototype()
    d, d0 = ShiftedBankDefinition(M, P, D, h, half), ShiftedBankDefinition(M, P, D, h, 0)
    cuts = [0, 7, 7 + D - 1, nin // 3, nin // 3 + 1, nin]
    e0 = e1 = 0.0
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        if i == 3:
            ch.set_shift(ODD_LARGE), d.set_shift(ODD_LARGE)
        yg, yd = ch.process(x[a:b]), d.process(x[a:b])
        yg0, yd0 = ch0.process(x[a:b]), d0.process(x[a:b])
        assert yg.shape == yd.shape
        if len(yd):
            e1 = max(e1, np.abs(yg - yd).max() / (np.abs(yd).max() + 1e-12))
            e0 = max(e0, np.abs(yg0 - yd0).max() / (np.abs(yd0).max() + 1e-12))
    print("chan_shift_error M %d P %d D %d nin %d flags %d: e0 %.3e e1 %.3e" % (M, P, D, nin, flags, e0, e1))
    assert e1 < 2e-5, (e0, e1)
    assert e0 < 2e-5, e0
    ch.close()
    ch0.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M,P,D,nin", SWEEP)
def test_gpu_shifted_geometry_sweep_matches_definition(pkg, oracle, M, P, D, nin):
    """test_chan.py's geometry sweep (D not dividing M, D > M, D = 1, P = 1 and 32, a factor of 1, the largest factors, M = 800 off
    the FFT kernel's geometry) under half a bin of shift from the first sample and ODD_LARGE from the call that ends a sample before
    a frame boundary on: the phasor inc n_m mod 2^32 and the modulated taps hang on the same per-frame indices as the fold.  Same
    chunking, same bound (2e-5 of the call's largest output, DESIGN.md section 8.8 with the measured values), same agreement of
    frames_for, the definition's count and the returned count."""
    rng = np.random.default_rng(1000 * M + 40 * D + P)
    x = _noise(rng, nin)
    half = TWO32 // (2 * M)
    ch = pkg.Channeliser(M, P, D, max_in=nin, shift=half)
    d = ShiftedBankDefinition(M, P, D, ch.prototype(), half)
    cuts = _sweep_cuts(M, P, D, nin)

    def process(a, b):
        if (a, b) == (cuts[-4], cuts[-3]):
            ch.set_shift(ODD_LARGE), d.set_shift(ODD_LARGE)
        return ch.process(x[a:b])

    err = _sweep_check(M, P, D, cuts, ch.frames_for, process, lambda a, b: d.process(x[a:b]),
                       lambda n: (d.buf.size - (d.L - 1) + n) // D - d.m)
    ch.close()
    print("chan_shift_sweep_error M %d P %d D %d nin %d: e1 %.3e" % (M, P, D, nin, err))
    assert err < 2e-5, err


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["int16", "int8"])
@pytest.mark.parametrize("M,P,D,flags", [(800, 8, 400, 0), (800, 6, 400, 0), (800, 8, 400, 2), (800, 8, 400, 1), (32, 8, 16, 0)])
def test_gpu_shifted_integer_input_matches_definition_and_the_float_route(pkg, oracle, M, P, D, flags, dtype):
    """The formats and geometries of test_chan.py's integer test under half a bin of shift: against the definition on the quantised
    samples (2e-5) and bit for bit the complex64 entry point on the converted samples; ragged chunks, formats mixed on one handle."""
    import torch
    dev = torch.device("cuda", 0)
    np_dtype = np.int16 if dtype == "int16" else np.int8
    rng = np.random.default_rng(M + P)
    nin = D * 150 + 11
    q, xq = _quantise(rng.standard_normal(nin) + 1j * rng.standard_normal(nin), np_dtype)
    half = TWO32 // (2 * M)
    ch_i = pkg.Channeliser(M, P, D, max_in=nin, flags=flags, shift=half)
    ch_f = pkg.Channeliser(M, P, D, max_in=nin, flags=flags, shift=half)
    d = ShiftedBankDefinition(M, P, D, ch_i.prototype(), half)
    d_q, d_x = torch.from_numpy(q).to(dev), torch.from_numpy(xq).to(dev)
    cuts = [0, 5, 5 + D - 1, nin // 3, nin // 3 + 2, nin]
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        yd = d.process(xq[a:b])
        out_i = torch.zeros((max(1, ch_i.frames_for(b - a)), M), dtype=torch.complex64, device=dev)
        out_f = torch.zeros_like(out_i)
        n_i = ch_i.process_device(d_x[a:b] if i == 3 else d_q[a:b], b - a, out_i)
        n_f = ch_f.process_device(d_x[a:b], b - a, out_f)
        torch.cuda.synchronize()
        assert n_i == n_f == len(yd)
        if n_i:
            assert torch.equal(out_i[:n_i], out_f[:n_f]), (a, b)
            err = np.abs(out_i[:n_i].cpu().numpy() - yd).max() / (np.abs(yd).max() + 1e-12)
            assert err < 2e-5, (a, b, err)
    ch_i.close()
    ch_f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("M,P,D,flags", [(800, 8, 400, 0), (800, 6, 400, 0), (800, 4, 400, 0), (800, 8, 400, 2), (800, 8, 400, 1), (32, 8, 16, 0)])
def test_gpu_shift_zero_equals_a_handle_that_never_set_a_shift(pkg, M, P, D, flags):
    """set_shift(0) -- directly, and after a non-zero shift was set and taken back -- runs the un-shifted kernels: torch.equal with a
    handle that never called set_shift, for complex64 and int16 input, ragged chunks."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(P)
    nin = D * 90 + 13
    q, xq = _quantise(rng.standard_normal(nin) + 1j * rng.standard_normal(nin), np.int16)
    plain, zero, back = (pkg.Channeliser(M, P, D, max_in=nin, flags=flags) for _ in range(3))
    zero.set_shift(0)
    back.set_shift(ODD_LARGE)
    back.set_shift(0)
    assert zero.get_shift() == 0 and back.get_shift() == 0
    d_q, d_x = torch.from_numpy(q).to(dev), torch.from_numpy(xq).to(dev)
    cuts = [0, 3, D + 1, nin // 2, nin]
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        src = d_q if i % 2 else d_x
        outs = []
        for ch in (plain, zero, back):
            out = torch.zeros((max(1, ch.frames_for(b - a)), M), dtype=torch.complex64, device=dev)
            n = ch.process_device(src[a:b], b - a, out)
            outs.append(out[:n])
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (a, b)
    for ch in (plain, zero, back):
        ch.close()
