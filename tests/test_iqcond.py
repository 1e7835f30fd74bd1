"""Conditioning of the capture in the wideband front end (include/ext/tetra_iqcond.h): the per-sample real affine map of (I, Q) inside the
channeliser's loads, the one-pass statistics of a capture and the closed-form solver.

The map has an exact contract (two chained fmaf per component on the converted sample), so the host build of the lane code
(tests/emul/iqcond_emul.cpp) is held to numpy bit for bit where the arithmetic is exact and to the rounding bound elsewhere, and the GPU is
held bit for bit to the un-conditioned channeliser fed the host-conditioned stream."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_SIZE, ERR_ALIGN = -1, -6, -7
IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
SWAP = (0.0, 1.0, 1.0, 0.0, 0.0, 0.0)
NEG_Q = (1.0, 0.0, 0.0, -1.0, 0.0, 0.0)
MAP_A = (1.0, 0.0, -0.0523, 0.953, 0.0123, -0.0045)         # the solver's kind: I alone, Q decorrelated and scaled, both offsets
MAP_B = (0.03, 1.5, -0.75, 0.01, -0.002, 0.003)             # swap-like with scales: every coefficient in use
G, PHI, DC = 1.05, math.radians(3.0), (0.011, -0.007)       # the impairment of the issue: gain, phase, offset (full scale = 1)


def _f64_eval(m, xr, xi):
    """(inner r, yr, inner i, yi) of the contract's expression in float64 from float32 inputs."""
    m = [np.float64(np.float32(v)) for v in m]
    xr, xi = xr.astype(np.float64), xi.astype(np.float64)
    ir, ii = m[0] * xr + m[4], m[2] * xr + m[5]
    return ir, m[1] * xi + ir, ii, m[3] * xi + ii


def _converted(x):
    if x.dtype == np.complex64:
        return x.real.copy(), x.imag.copy()
    full = np.float32(32768.0 if x.dtype == np.int16 else 128.0)
    return x[:, 0].astype(np.float32) / full, x[:, 1].astype(np.float32) / full


def _samples(rng, dtype, n):
    if dtype == np.complex64:      # on the cs16 grid, so that an integer DC stays exact; magnitudes up to 4
        return ((rng.integers(-131072, 131072, n) + 1j * rng.integers(-131072, 131072, n)) / 32768.0).astype(np.complex64)
    info = np.iinfo(dtype)
    x = rng.integers(info.min, info.max + 1, (n, 2)).astype(dtype)
    x[0], x[1] = (info.min, info.max), (info.max, info.min)
    return x


def _impair(z, g=G, phi=PHI, dc=DC):
    """I' = I + dI, Q' = g (Q cos phi + I sin phi) + dQ, in the precision of z."""
    return (z.real + dc[0]) + 1j * (g * (z.imag * math.cos(phi) + z.real * math.sin(phi)) + dc[1])


# ---------------------------------------------------------------------------------------------------------------------- CPU


@pytest.mark.parametrize("dtype", [np.int16, np.int8, np.complex64])
def test_exact_maps_on_the_host_equal_numpy_bit_for_bit(dtype):
    """Identity, I / Q swap, Q negation, power-of-two scales and an integer DC offset: every product and sum is exact in binary32 on these
    inputs, so the lane code must give the float64 evaluation's value to the bit (the signs of zeros included: a fused multiply-add and
    the float64 expression obey the same rule for them)."""
    from tests.emul import iqcond_emul_bind as E
    rng = np.random.default_rng(5)
    x = _samples(rng, dtype, 4099)
    lsb = 1.0 / (128.0 if dtype == np.int8 else 32768.0)
    maps = [IDENTITY, SWAP, NEG_Q, (2.0, 0.0, 0.0, 0.5, 0.0, 0.0), (0.0, -4.0, 0.25, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 1.0, -37 * lsb, 101 * lsb),
            (0.0, 1.0, -1.0, 0.0, 5 * lsb, -3 * lsb)]
    xr, xi = _converted(x)
    for m in maps:
        got = E.apply(x, m)
        _, yr, _, yi = _f64_eval(m, xr, xi)
        assert np.array_equal(yr.astype(np.float32).astype(np.float64), yr) and np.array_equal(yi.astype(np.float32).astype(np.float64), yi), m   # exact indeed
        assert np.array_equal(got.real.view(np.uint32), yr.astype(np.float32).view(np.uint32)), (dtype, m)
        assert np.array_equal(got.imag.view(np.uint32), yi.astype(np.float32).view(np.uint32)), (dtype, m)


@pytest.mark.parametrize("dtype", [np.int16, np.int8, np.complex64])
def test_general_maps_on_the_host_are_within_one_ulp_of_float64(dtype):
    """Two chained roundings: the inner fmaf is off by at most half an ulp of its result, the outer by half an ulp of its own, so the
    component is within ONE ulp -- taken at the larger of the inner and the final magnitude -- of the float64 evaluation (whose own
    error, 2^-53 relative, is far below).  The bound is that derivation, not a measurement."""
    from tests.emul import iqcond_emul_bind as E
    rng = np.random.default_rng(6)
    x = _samples(rng, dtype, 20011)
    xr, xi = _converted(x)
    for m in (MAP_A, MAP_B, (0.999, 0.017, -0.05, 1.04, 1e-3, -2e-3), (-1.7, 0.3, 0.9, 2.2, 0.5, -0.25)):
        got = E.apply(x, m)
        ir, yr, ii, yi = _f64_eval(m, xr, xi)
        for g, inner, y in ((got.real, ir, yr), (got.imag, ii, yi)):
            ulp = np.spacing(np.maximum(np.abs(inner), np.abs(y)).astype(np.float32)).astype(np.float64)
            assert np.all(np.abs(g.astype(np.float64) - y) <= ulp), (dtype, m)


def _numpy_solver(n, s_i, s_q, s_ii, s_qq, s_iq):
    """The header's formula in numpy float64, operation by operation; None where it refuses."""
    f = np.float64
    n, s_i, s_q, s_ii, s_qq, s_iq = f(n), f(s_i), f(s_q), f(s_ii), f(s_qq), f(s_iq)
    uI, uQ = s_i / n, s_q / n
    A, B, Cc = s_ii / n - uI * uI, s_qq / n - uQ * uQ, s_iq / n - uI * uQ
    if n < 2 or not A > 0:
        return None
    den = B - Cc * Cc / A
    if not den > 0:
        return None
    r, k = Cc / A, np.sqrt(A / den)
    return tuple(float(np.float32(v)) for v in (1.0, 0.0, -(k * r), k, -uI, k * (r * uI - uQ)))


def _int_stats(q):
    """(n, s_i, s_q, s_ii, s_qq, s_iq) of an integer capture [n][2]: exact int64 sums, converted and scaled."""
    sh = 15 if q.dtype == np.int16 else 7
    i, qq = q[:, 0].astype(np.int64), q[:, 1].astype(np.int64)
    sums = [int(i.sum()), int(qq.sum()), int((i * i).sum()), int((qq * qq).sum()), int((i * qq).sum())]
    return (q.shape[0],) + tuple(math.ldexp(float(np.float64(np.int64(v))), -(sh if j < 2 else 2 * sh)) for j, v in enumerate(sums))


def test_solver_equals_the_formula_in_numpy_float64(pkg):
    rng = np.random.default_rng(7)
    for trial in range(40):
        n = int(rng.integers(2, 1 << 20))
        z = rng.standard_normal(64) + 1j * rng.standard_normal(64)
        y = _impair(z * rng.uniform(0.01, 0.3), rng.uniform(0.8, 1.25), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1, 2))
        st = (n, y.real.sum() * n / 64, y.imag.sum() * n / 64, (y.real ** 2).sum() * n / 64, (y.imag ** 2).sum() * n / 64, (y.real * y.imag).sum() * n / 64)
        want = _numpy_solver(*st)
        assert want is not None
        got = pkg.input_map_from_stats(st)
        assert np.array_equal(np.array(got, np.float32).view(np.uint32), np.array(want, np.float32).view(np.uint32)), (trial, got, want)
        assert got[0] == 1.0 and got[1] == 0.0


def test_solver_refuses_what_has_no_answer(pkg):
    L = pkg.chan_binding._lib()
    S, Mp = pkg.chan_binding.IqStats, pkg.chan_binding.IqMap
    m = Mp()
    ok = S(4, 0.0, 0.0, 4.0, 4.0, 0.0)                           # I = (1, -1, 1, -1), Q = (1, 1, -1, -1)
    assert L.tetra_iq_map_from_stats(C.byref(ok), C.byref(m)) == 0 and m.astuple() == (1.0, 0.0, -0.0, 1.0, -0.0, 0.0)
    for bad in (S(1, 0.5, 0.5, 0.25, 0.25, 0.25), S(0, 0, 0, 0, 0, 0), S(-3, 0, 0, 1, 1, 0),      # n < 2
                S(4, 2.0, 0.0, 1.0, 4.0, 0.0),                   # constant I = 0.5: A = 0
                S(4, 0.0, 0.0, 4.0, 4.0, 4.0),                   # Q = I: B - C^2 / A = 0
                S(4, 0.0, 0.0, 4.0, 16.0, -8.0),                 # Q = -2 I
                S(4, float("nan"), 0.0, 4.0, 4.0, 0.0)):
        m = Mp(9, 9, 9, 9, 9, 9)
        assert L.tetra_iq_map_from_stats(C.byref(bad), C.byref(m)) == ERR_ARG, bad.astuple()
        assert m.astuple() == (9.0,) * 6
        assert bad.n < 2 or _numpy_solver(*bad.astuple()) is None
    assert L.tetra_iq_map_from_stats(None, C.byref(m)) == ERR_ARG and L.tetra_iq_map_from_stats(C.byref(ok), None) == ERR_ARG
    with pytest.raises(pkg.TetraDemodError) as e:
        pkg.input_map_from_stats((4, 0.0, 0.0, 4.0, 4.0, 4.0))
    assert e.value.status == ERR_ARG


def _band_noise(rng, n, half_width):
    """Circular complex Gaussian noise (proper) confined to |f| < half_width cycles per sample, unit power; float64."""
    w = np.fft.fft(rng.standard_normal(n) + 1j * rng.standard_normal(n))
    w[np.abs(np.fft.fftfreq(n)) >= half_width] = 0
    s = np.fft.ifft(w)
    return s / np.sqrt(np.mean(np.abs(s) ** 2))


IMAGE_N = 1 << 18


def _image_dbc(y, parts):
    """Joint least-squares projection of y (complex128) onto every carrier, every carrier's mirror image and a constant: the strong
    carrier's image coefficient against its direct one, in dB."""
    cols = [p for p in parts] + [np.conj(p) for p in parts] + [np.ones_like(parts[0])]
    coef = np.linalg.lstsq(np.stack(cols, 1), y, rcond=None)[0]
    return 20 * math.log10(abs(coef[len(parts)]) / abs(coef[0]))


def test_estimated_map_takes_the_strong_carriers_image_below_minus_60_dbc(pkg):
    """A proper capture at 32 bins' rate -- a strong carrier on bin 1, one 30 dB weaker on its mirror bin 31, a third on bin 7, each 18
    kHz of circular noise -- with g = 1.05, phi = 3 degrees and a DC offset applied in float64, quantised to cs16, 2^18 samples.  Raw,
    the strong carrier's image stands at -29 dBc (on top of the weak carrier); after the map solved from the capture's own exact sums and
    applied by the lane code it must be at or below -60 dBc.  Measured with this signal: -78.4 dBc (raw -28.9): 18 dB of margin."""
    from tests.emul import iqcond_emul_bind as E
    rng = np.random.default_rng(2024)
    n = IMAGE_N
    t = np.arange(n)
    parts = [a * _band_noise(rng, n, 9e3 / 800e3) * np.exp(2j * np.pi * k / 32 * t) for k, a in ((1, 1.0), (-1, 10 ** (-30 / 20)), (7, 0.5))]
    z = sum(parts)
    z = z * (0.25 / np.abs(z).max())
    parts = [p * (0.25 / np.abs(sum(parts)).max()) for p in parts]
    y = _impair(z)
    q = np.stack([np.round(y.real * 32768), np.round(y.imag * 32768)], 1).astype(np.int16)
    raw = (q[:, 0] + 1j * q[:, 1]) / 32768.0
    raw_dbc = _image_dbc(raw, parts)
    assert -31 < raw_dbc < -27, raw_dbc
    m = pkg.input_map_from_stats(_int_stats(q))
    assert m == _numpy_solver(*_int_stats(q))
    # the exact inverse of the impairment, for orientation: m10 = -tan(phi), m11 = 1 / (g cos(phi)), c0 = -dI
    assert abs(m[2] + math.tan(PHI)) < 2e-3 and abs(m[3] - 1 / (G * math.cos(PHI))) < 2e-3 and abs(m[4] + DC[0]) < 1e-4
    out = E.apply(q, m).astype(np.complex128)
    dbc = _image_dbc(out, parts)
    print("iqcond image: raw %.1f dBc, conditioned %.1f dBc" % (raw_dbc, dbc))
    assert dbc <= -60, dbc
    assert abs(out.mean()) < 1e-6                                 # the DC offset is gone (the estimate's own mean, to float32 rounding)


def test_iqcond_header_is_exported_bound_and_laid_out_as_the_ctypes_mirrors(pkg):
    """tests/test_abi.py's rule for the extension header: every function it declares is exported and has an entry with as many parameters
    in a binding module's IQCOND_ABI table; the header compiles as C; both structs have the size and the offsets of their ctypes mirrors."""
    hdr = os.path.join(ROOT, "include", "ext", "tetra_iqcond.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): m.group(2).split(",") for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    tables = {**pkg.chan_binding.IQCOND_ABI, **pkg.wbrx_binding.IQCOND_ABI}
    assert len(decls) == 6 and set(decls) == set(tables)
    L = pkg.load_library()
    pkg.chan_binding._lib(), pkg.wbrx_binding._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        assert len(tables[name][1]) == len(params) == len(fn.argtypes), name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    mf, sf = ["m00", "m01", "m10", "m11", "c0", "c1"], ["n", "s_i", "s_q", "s_ii", "s_qq", "s_iq"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ext/tetra_iqcond.h"\nint main(){printf("%zu", sizeof(tetra_iq_map_t));' +
            "".join('printf(" %%zu", offsetof(tetra_iq_map_t, %s));' % f for f in mf) + 'printf(" %zu", sizeof(tetra_iq_stats_t));' +
            "".join('printf(" %%zu", offsetof(tetra_iq_stats_t, %s));' % f for f in sf) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "s.c"), "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), os.path.join(td, "s.c"), "-o", os.path.join(td, "s")], check=True)
        got = list(map(int, subprocess.run([os.path.join(td, "s")], check=True, capture_output=True, text=True).stdout.split()))
    Mp, S = pkg.chan_binding.IqMap, pkg.chan_binding.IqStats
    assert got == [C.sizeof(Mp)] + [getattr(Mp, f).offset for f in mf] + [C.sizeof(S)] + [getattr(S, f).offset for f in sf]
    assert C.sizeof(Mp) == 24 and C.sizeof(S) == 48
    assert (pkg.chan_binding.IQ_FMT_C64, pkg.chan_binding.IQ_FMT_CS16, pkg.chan_binding.IQ_FMT_CS8) == (0, 1, 2)
    assert all(("#define TETRA_IQ_FMT_%s %d" % (n, v)) in open(hdr).read() for n, v in (("C64", 0), ("CS16", 1), ("CS8", 2)))


def test_input_map_entry_points_refuse_null_handles_without_a_gpu(pkg):
    L = pkg.chan_binding._lib()
    pkg.wbrx_binding._lib()
    m, on = pkg.chan_binding.IqMap(*IDENTITY), C.c_int(7)
    for name in ("tetra_chan", "tetra_wbrx"):
        assert getattr(L, name + "_set_input_map")(None, C.byref(m)) == ERR_ARG
        assert getattr(L, name + "_set_input_map")(None, None) == ERR_ARG
        assert getattr(L, name + "_get_input_map")(None, C.byref(m), C.byref(on)) == ERR_ARG
    assert on.value == 7
    st = pkg.chan_binding.IqStats()
    assert L.tetra_iq_stats_device(None, 1, 0, None, None) == ERR_ARG
    assert L.tetra_iq_stats_device(None, 3, 0, C.byref(st), None) == ERR_ARG and L.tetra_iq_stats_device(None, -1, 0, C.byref(st), None) == ERR_ARG
    assert L.tetra_iq_stats_device(None, 1, 5, C.byref(st), None) == ERR_ARG and L.tetra_iq_stats_device(None, 1, -1, C.byref(st), None) == ERR_SIZE
    st.n = 9
    assert L.tetra_iq_stats_device(None, 0, 0, C.byref(st), None) == 0 and st.astuple() == (0, 0.0, 0.0, 0.0, 0.0, 0.0)      # n = 0 needs no device
    with pytest.raises(ValueError):
        pkg.chan_binding.as_iq_map((1, 0, 0, 1))


# ---------------------------------------------------------------------------------------------------------------------- GPU

CHAN_GEOMETRIES = [(800, 8, 400, 0, 16137), (800, 8, 400, 2, 16137), (32, 8, 16, 0, 16 * 61 + 5), (32, 8, 16, 1, 16 * 61 + 5)]


def _bits(torch, t):
    return torch.view_as_real(t).view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("shift_on", [False, True])
@pytest.mark.parametrize("dtype", [np.complex64, np.int16, np.int8])
@pytest.mark.parametrize("M,P,D,flags,nin", CHAN_GEOMETRIES)
def test_gpu_conditioned_channeliser_equals_the_plain_one_on_the_host_conditioned_stream(pkg, M, P, D, flags, nin, dtype, shift_on):
    """chan(map, x) against chan(no map, complex64 of the host lane code's map(x)), bit for bit: the FFT kernel (in-place fold and
    conditioned carry), the matrix and the direct kernel (conditioned staging), each sample format, shift off and half a bin.  Calls:
    map A, map B (the delay line then holds A's samples: the 'map of the delivering call' rule), no map, then map A on a call shorter
    than D (a carry that keeps most of the line), then B again.  n_in = 16137 gives the FFT kernel careful first blocks, blocks that read
    only new samples and a ragged last one."""
    import torch
    from tests.emul import iqcond_emul_bind as E
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(M + P + flags)
    short = D - 3
    lens = [nin, nin, nin, short, nin]
    maps = [MAP_A, MAP_B, None, MAP_A, MAP_B]
    if dtype == np.complex64:
        x = (0.3 * (rng.standard_normal(sum(lens)) + 1j * rng.standard_normal(sum(lens)))).astype(np.complex64)
    else:
        x = _samples(rng, dtype, sum(lens))
    shift = (1 << 32) // (2 * M) if shift_on else 0
    a = pkg.Channeliser(M, P, D, max_in=nin, flags=flags, shift=shift)
    b = pkg.Channeliser(M, P, D, max_in=nin, flags=flags, shift=shift)
    assert a.get_input_map() is None
    at = 0
    frames = 0
    for n, m in zip(lens, maps):
        part = x[at:at + n]
        at += n
        a.set_input_map(m)
        assert a.get_input_map() == (None if m is None else tuple(float(np.float32(v)) for v in m)) and b.get_input_map() is None
        if m is None:
            xr, xi = _converted(part)
            host = (xr + 1j * xi).astype(np.complex64)
        else:
            host = E.apply(part, m)
        d_a, d_b = torch.from_numpy(part).to(dev), torch.from_numpy(host).to(dev)
        out_a = torch.zeros((max(1, a.frames_for(n)), M), dtype=torch.complex64, device=dev)
        out_b = torch.full_like(out_a, float("nan"))
        n_a, n_b = a.process_device(d_a, n, out_a), b.process_device(d_b, n, out_b)
        torch.cuda.synchronize()
        assert n_a == n_b
        frames += n_a
        assert torch.equal(_bits(torch, out_a[:n_a]), _bits(torch, out_b[:n_b])), (n, m)
    assert frames == sum(lens) // D
    a.reset()                                   # a reset keeps the map, as it keeps the shift
    assert a.get_input_map() == tuple(float(np.float32(v)) for v in MAP_B)
    a.close()
    b.close()


STATS_NS = [1, 255, 256, 257, (1 << 20) + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int16, np.int8])
def test_gpu_integer_statistics_are_the_exact_sums(pkg, dtype):
    """cs16 / cs8: every field equals the numpy int64 sum, converted to float64 and scaled by the power of two -- bit for bit, at sizes
    around one workgroup, a size that makes the lanes loop, and on a buffer of nothing but the most negative value."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    big = _samples(rng, dtype, STATS_NS[-1])
    low = np.full((STATS_NS[-1], 2), np.iinfo(dtype).min, dtype)
    for buf in (big, low):
        d = torch.from_numpy(buf).to(dev)
        for n in STATS_NS:
            got = pkg.iq_stats(d[:n]).astuple()
            want = _int_stats(buf[:n])
            assert got[0] == n and np.array_equal(np.array(got[1:]).view(np.uint64), np.array(want[1:]).view(np.uint64)), (n, got, want)
    assert pkg.iq_stats(torch.from_numpy(big).to(dev), n=0).astuple() == (0, 0.0, 0.0, 0.0, 0.0, 0.0)


@pytest.mark.gpu
def test_gpu_complex64_statistics_are_within_the_summation_bound_and_repeat(pkg):
    """complex64: every term is exact in float64, so only the additions round: any order of n terms is within (n - 1) 2^-53 sum |term| of
    the exact sum to first order, and numpy's pairwise float64 sum well inside that -- n 2^-53 sum |term| between the two is the derived
    worst case with room for numpy's own error.  Two calls give the same bits."""
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(10)
    n_max = STATS_NS[-1]
    x = ((rng.standard_normal(n_max) + 0.3) + 1j * (rng.standard_normal(n_max) * 2 - 0.1)).astype(np.complex64)
    d = torch.from_numpy(x).to(dev)
    for n in STATS_NS:
        got, again = pkg.iq_stats(d[:n]).astuple(), pkg.iq_stats(d[:n]).astuple()
        assert got == again and got[0] == n
        i, q = x[:n].real.astype(np.float64), x[:n].imag.astype(np.float64)
        for g, term in zip(got[1:], (i, q, i * i, q * q, i * q)):
            bound = n * 2.0 ** -53 * np.abs(term).sum()
            assert abs(g - term.sum()) <= bound, (n, g, term.sum(), bound)


# ---- end to end on the wideband receiver: 32 bins at 800 kHz, D 16, 80 slots, cs16 ---------------------------------------------------------
WB_M, WB_D, WB_SLOTS = 32, 16, 80
WB_BINS = [1, 7, 31]
WB_CARRIERS = {1: (11, 0.0), 7: (12, -6.0), 31: (14, -30.0)}      # bin: (seed, level in dB): the weak carrier sits on the strong one's mirror bin
WB_WEAK = WB_BINS.index(31)
EST_N = 1 << 18


def _capture128(torch, synth, M, carriers, nslots, seed=1, noise=1e-3):
    """tests/test_wbrx.py::_capture with a level per carrier, kept in complex128 (peak 0.25) for the impairment ahead of the quantiser."""
    dev = torch.device("cuda")
    fs = M * 25000.0
    N = (nslots * 510 - 100) // 9 * 9
    L = int(round(N * fs / 36000.0))
    x = torch.zeros(L, dtype=torch.complex128, device=dev)
    n = torch.arange(L, dtype=torch.float64, device=dev)
    cells, tx = {}, {}
    for k, (sd, level_db) in carriers.items():
        cells[k] = (100 + 7 * sd % 900, 1000 + 13 * sd, (5 + 3 * sd) % 64)
        tx[k] = synth.gen_downlink(nslots, sd, cell=cells[k])
        s = torch.from_numpy(synth.gen_channel(N, sd + 100, bits=tx[k][0], amp=1.0)[0].astype(np.complex128)).to(dev)
        S = torch.fft.fft(s)
        Y = torch.zeros(L, dtype=torch.complex128, device=dev)
        Y[: N // 2] = S[: N // 2]
        Y[L - (N - N // 2):] = S[N // 2:]
        y = torch.fft.ifft(Y) * (L / N)
        kc = k if k < M // 2 else k - M
        x += 10.0 ** (level_db / 20.0) * y * torch.polar(torch.ones_like(n), 2.0 * math.pi * kc / M * n)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x += noise * torch.view_as_complex(torch.randn((L, 2), device=dev, generator=g, dtype=torch.float64))
    x *= 0.25 / float(x.abs().max())
    return x, cells, tx


def _quantise16(torch, x):
    return torch.view_as_real(x).mul(32768.0).round().clamp(-32768, 32767).to(torch.int16).contiguous()


@pytest.fixture(scope="module")
def mirror_capture(pkg, synth):
    """(clean cs16, impaired cs16, cells, tx): the impairment -- g, phi, DC -- applied in float64 before the quantiser."""
    import torch
    x, cells, tx = _capture128(torch, synth, WB_M, WB_CARRIERS, WB_SLOTS)
    bad = torch.complex(x.real + DC[0], G * (x.imag * math.cos(PHI) + x.real * math.sin(PHI)) + DC[1])
    return _quantise16(torch, x), _quantise16(torch, bad), cells, tx


def _run(pkg, xs, m=None, estimate=False):
    from tests.test_wbrx import _run_collect
    wb = pkg.WidebandRx(WB_BINS, n_channels=WB_M, decimation=WB_D, max_in=xs.shape[0])
    if estimate:
        m = wb.estimate_input_map(xs[:EST_N])
        assert wb.get_input_map() == m
    elif m is not None:
        wb.set_input_map(m)
    got = _run_collect(pkg, wb, xs, [0, xs.shape[0]])
    cell = wb.rx.cells()
    wb.close()
    return got, cell, m


def _assert_weak_carrier_known_answer(pkg, synth, got, cell, cells, tx):
    """tests/test_wbrx.py::_assert_known_answer for the weak carrier's slot: behind acquisition (slot 28 on) every block of every kind
    is CRC-good and carries the type-1 bits that were sent in the slot its TDMA time names."""
    R = pkg.rx_binding
    names = {R.KIND_SB1: "sb1", R.KIND_BBK: "bbk", R.KIND_SB2: "sb2", R.KIND_NDB1: "ndb1", R.KIND_NDB2: "ndb2", R.KIND_SCH_F: "schf"}
    by_time = {}
    for s in range(WB_SLOTS):
        tn, fn, mn = synth.tdma_time_of_slot(s)
        by_time[tn | fn << 8 | mn << 16] = s
    c, k = WB_WEAK, WB_BINS[WB_WEAK]
    assert (cell[c].mcc, cell[c].mnc, cell[c].colour_code) == cells[k]
    good_sb1 = [r[1] for r in got[R.KIND_SB1] if r[0] == c and r[2]]
    assert good_sb1, "the weak carrier never locked"
    first, exact = min(good_sb1), 0
    for kind, name in names.items():
        sent = {s: v.tobytes() for s, v in tx[k][1][name]}
        rows = [r for r in got[kind] if r[0] == c and r[1] > first]
        assert len(rows) >= {"sb1": 8, "sb2": 8, "ndb1": 8, "ndb2": 8, "schf": 20, "bbk": 50}[name], (name, len(rows))
        for ch, bitnum, ok, t_rx, t, bits in rows:
            if bitnum < 28 * 510:
                continue
            assert ok == 1 and t in by_time, (name, bitnum, hex(t))
            assert sent[by_time[t]] == bits, (name, by_time[t])
            exact += 1
    assert exact >= 5 * (WB_SLOTS - 32) // 2, exact


def _good_schf(pkg, got):
    return len([r for r in got[pkg.rx_binding.KIND_SCH_F] if r[0] == WB_WEAK and r[2]])


@pytest.mark.gpu
def test_gpu_wbrx_weak_carrier_on_the_mirror_bin_with_and_without_the_estimated_map(pkg, synth, mirror_capture):
    """(a) the clean capture, no map: the carrier 30 dB under the one on its mirror bin decodes to the known answer -- the scenario
    holds at -30 dB as the issue states it.  (b) g = 1.05, phi = 3 degrees and DC ahead of the quantiser, estimate_input_map on the first
    2^18 samples: the same known answer.  (c) as (b) without a map: the strong carrier's image (-29 dBc) lies on the weak carrier, and
    strictly fewer of its SCH/F blocks are CRC-good.  (d) the clean capture with Q inverted and the map {1, 0, 0, -1, 0, 0}: the rows of
    (a), bit for bit."""
    import torch
    clean, bad, cells, tx = mirror_capture
    got_a, cell_a, _ = _run(pkg, clean)
    _assert_weak_carrier_known_answer(pkg, synth, got_a, cell_a, cells, tx)
    got_b, cell_b, m = _run(pkg, bad, estimate=True)
    assert abs(m[2] + math.tan(PHI)) < 5e-3 and abs(m[3] - 1 / (G * math.cos(PHI))) < 5e-3 and abs(m[4] + DC[0]) < 1e-3, m
    _assert_weak_carrier_known_answer(pkg, synth, got_b, cell_b, cells, tx)
    got_c, _, _ = _run(pkg, bad)
    print("iqcond wbrx: CRC-good SCH/F of the weak carrier: clean %d, impaired + map %d, impaired %d" % (_good_schf(pkg, got_a), _good_schf(pkg, got_b), _good_schf(pkg, got_c)))
    assert _good_schf(pkg, got_c) < _good_schf(pkg, got_b)
    # (d) mirrored spectrum
    inv = clean.clone()
    inv[:, 1] = -inv[:, 1]
    got_d, cell_d, _ = _run(pkg, inv, m=NEG_Q)
    assert got_d == got_a and [bytes(c) for c in cell_d] == [bytes(c) for c in cell_a]
    torch.cuda.synchronize()


from tests.test_wbrx import small_capture  # noqa: E402,F401  (the fixture of test_gpu_wbrx_equals_the_hand_wired_composition)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["c64", "cs16"])
def test_gpu_no_map_ever_and_null_after_a_map_equal_a_handle_that_never_heard_of_it(pkg, small_capture, fmt):
    """test_gpu_wbrx_equals_the_hand_wired_composition's capture and cuts: a handle that set a map and took it back before its first call,
    and one that processes the first cuts WITH a map on a side stream of calls and is then reset, against a plain handle -- resampled
    frames, rows and bit rows equal after every call; the plain handle itself is pinned to the hand-wired composition by that test."""
    import torch
    from tests.chain_gpu import bit_rows as _bit_rows
    from tests.test_wbrx import BINS_SMALL, D_SMALL, M_SMALL, _cs16, _rows
    R = pkg.rx_binding
    x = small_capture[0]
    xin = x if fmt == "c64" else _cs16(torch, x)
    L = x.shape[0]
    cuts = [0, 5, 5 + 9, 200003, 200003 + 16 * 1000 + 7, 470000, 470010, 700001, L]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    plain, back, used = (pkg.WidebandRx(BINS_SMALL, n_channels=M_SMALL, decimation=D_SMALL, max_in=max_in) for _ in range(3))
    back.set_input_map(MAP_A)
    back.set_input_map(None)
    used.set_input_map(MAP_B)
    used.process_device(xin[:20000], 20000)
    used.set_input_map(None)
    used.reset()
    assert plain.get_input_map() is None and back.get_input_map() is None and used.get_input_map() is None
    s = torch.cuda.current_stream()
    for a, b in zip(cuts, cuts[1:]):
        for wb in (plain, back, used):
            wb.process_device(xin[a:b], b - a, s)
        want = _bits(torch, plain.frames())
        for wb in (back, used):
            assert torch.equal(_bits(torch, wb.frames()), want), (a, b)
            assert _rows(wb.rx, R) == _rows(plain.rx, R), (a, b)
            assert _bit_rows(torch, wb.rx, 4) == _bit_rows(torch, plain.rx, 4), (a, b)
        torch.cuda.synchronize()
    for wb in (plain, back, used):
        wb.close()


@pytest.mark.gpu
def test_gpu_iqcond_statuses(pkg):
    import torch
    L = pkg.chan_binding._lib()
    pkg.wbrx_binding._lib()
    Mp, S = pkg.chan_binding.IqMap, pkg.chan_binding.IqStats
    ch = pkg.Channeliser(32, 8, 16, max_in=1000)
    wb = pkg.WidebandRx([1, 7], n_channels=32, decimation=16, max_in=1000)
    ch.set_input_map(MAP_A)
    wb.set_input_map(MAP_B)
    for i in range(6):
        for v in (float("nan"), float("inf"), -float("inf")):
            vals = list(IDENTITY)
            vals[i] = v
            m = Mp(*vals)
            assert L.tetra_chan_set_input_map(ch._h, C.byref(m)) == ERR_ARG and L.tetra_wbrx_set_input_map(wb._h, C.byref(m)) == ERR_ARG
            with pytest.raises(pkg.TetraDemodError) as e:
                ch.set_input_map(vals)
            assert e.value.status == ERR_ARG
    f32 = lambda m: tuple(float(np.float32(v)) for v in m)      # noqa: E731
    assert ch.get_input_map() == f32(MAP_A) and wb.get_input_map() == f32(MAP_B)          # a refused map leaves the one in force
    assert L.tetra_chan_get_input_map(ch._h, None, None) == ERR_ARG and L.tetra_wbrx_get_input_map(wb._h, None, None) == ERR_ARG
    m = Mp()
    assert L.tetra_chan_get_input_map(ch._h, C.byref(m), None) == 0 and m.astuple() == f32(MAP_A)
    ch.set_input_map(None)
    on = C.c_int(5)
    assert L.tetra_chan_get_input_map(ch._h, C.byref(m), C.byref(on)) == 0 and on.value == 0 and m.astuple() == IDENTITY
    # statistics: format, alignment, NULL
    raw = torch.zeros(4096 + 16, dtype=torch.uint8, device="cuda")
    st = S()
    p = raw.data_ptr()
    assert L.tetra_iq_stats_device(C.c_void_p(p), 3, 100, C.byref(st), None) == ERR_ARG
    assert L.tetra_iq_stats_device(C.c_void_p(p), -1, 100, C.byref(st), None) == ERR_ARG
    assert L.tetra_iq_stats_device(C.c_void_p(p), 1, 100, None, None) == ERR_ARG
    assert L.tetra_iq_stats_device(None, 1, 100, C.byref(st), None) == ERR_ARG
    assert L.tetra_iq_stats_device(C.c_void_p(p), 1, -1, C.byref(st), None) == ERR_SIZE
    assert L.tetra_iq_stats_device(C.c_void_p(p), 1, (1 << 32) + 1, C.byref(st), None) == ERR_SIZE
    assert L.tetra_iq_stats_device(C.c_void_p(p + 4), 0, 100, C.byref(st), None) == ERR_ALIGN
    assert L.tetra_iq_stats_device(C.c_void_p(p + 2), 1, 100, C.byref(st), None) == ERR_ALIGN
    assert L.tetra_iq_stats_device(C.c_void_p(p + 1), 2, 100, C.byref(st), None) == ERR_ALIGN
    assert L.tetra_iq_stats_device(C.c_void_p(p + 2), 2, 100, C.byref(st), None) == 0 and st.astuple() == (100, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert L.tetra_iq_stats_device(C.c_void_p(p + 4), 1, 100, C.byref(st), torch.cuda.current_stream().cuda_stream) == 0 and st.n == 100
    # a capture the solver refuses leaves the handle's map alone
    with pytest.raises(pkg.TetraDemodError) as e:
        wb.estimate_input_map(torch.zeros((500, 2), dtype=torch.int16, device="cuda"))
    assert e.value.status == ERR_ARG and wb.get_input_map() == f32(MAP_B)
    ch.close()
    wb.close()
