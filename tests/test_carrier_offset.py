"""Per-carrier frequency offsets in the selecting resampler (include/ext/tetra_carrier_offset.h) without a GPU: the host build of the
mixing thread code (tests/emul/resamp_mix_emul.cpp over csrc/resamp_core.hpp's MixColumns) against the double-precision definition
written out here in numpy, at any stream position; with all offsets zero bit for bit against the picking emulation; offsets that
change in mid-stream; and the header's entry points (exported, bound, refusing what they must)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -3
TOL = 2e-5                      # of the output's maximum: the project's bound for this family (tetra_shift.h, tests/test_chan_shift.py)
ODD_LARGE = 0x9E3779B1
INCS = [1, 2 ** 32 - 1, 2 ** 32 // 8, ODD_LARGE, 0]      # (2^32 / 8: an exact eighth of a turn per frame; one slot at 0 among the others)


def definition(x, first_frame, cols, inc, h, I, DN, T, m0, m1):
    """y[m][j] = sum_{t<T} h[r_m + I t] x[q_m - t][cols[j]] exp(-j 2 pi ((inc_j (q_m - t)) mod 2^32) / 2^32), I q_m + r_m = DN m, for
    m in [m0, m1), in float64.  x [n][M] holds the frames first_frame .. first_frame + n - 1; every frame before them is zero."""
    cols, inc = np.asarray(cols), np.asarray(inc, np.uint64)
    n = x.shape[0]
    a = (np.arange(first_frame - (T - 1), first_frame + n, dtype=np.int64) % (1 << 32)).astype(np.uint64)       # absolute frame index mod 2^32
    ph = (a[:, None] * inc[None, :]) & np.uint64(0xffffffff)                                                    # exact: < 2^64
    z = np.zeros((T - 1 + n, cols.size), np.complex128)
    z[T - 1:] = x[:, cols].astype(np.complex128)
    z *= np.exp(-2j * np.pi * ph.astype(np.float64) / 4294967296.0)
    m = np.arange(m0, m1, dtype=np.int64)
    q = DN * m // I
    r = DN * m - q * I
    y = np.zeros((m.size, cols.size), np.complex128)
    hd = np.asarray(h, np.float64)
    for t in range(T):
        y += hd[r + I * t][:, None] * z[q - t - first_frame + (T - 1)]
    return y


def _cases():
    from tests.emul import resamp_emul_bind as re_
    return [(I, DN, T, False) for I, DN, T in re_.ratios()] + [(18, 25, 16, True), (5, 7, 11, True)]


def _cuts(rng, n, DN, T):
    cuts = sorted(set([0, 1, 3, DN - 1, DN + 2, T - 2, T + 5, 3 * DN + 1, int(rng.integers(4 * DN, n)), n]))
    return [0, 0] + [c for c in cuts if 0 < c <= n] + [n]          # empty calls at both ends; calls shorter than DN and than T - 1 frames


def _run_against_definition(oracle, I, DN, T, generic, first_frame, inc_list, seed):
    from tests.emul import resamp_mix_emul_bind as me
    M = 32
    proto = oracle.ResampOracle(M, I, DN, T).h
    rng = np.random.default_rng(seed)
    n = 40 * DN + 13
    x = (rng.standard_normal((n, M)) + 1j * rng.standard_normal((n, M))).astype(np.complex64)
    worst = 0.0
    for trial in range(3):
        cols = rng.permutation(M)[: int(rng.integers(len(inc_list), M + 1))].astype(np.int32)
        inc = [inc_list[(j + trial) % len(inc_list)] if j < 2 * len(inc_list) else int(rng.integers(0, 2 ** 32)) for j in range(cols.size)]
        em = me.ResampMixEmul(M, cols, inc, I, DN, T, proto, generic=generic, first_frame=first_frame)
        m0 = em.m_next
        cuts = _cuts(rng, n, DN, T)
        got = np.concatenate([em.process(x[a:b]) for a, b in zip(cuts, cuts[1:])])
        assert not np.isnan(got.view(np.float32)).any()
        want = definition(x, first_frame, cols, inc, proto, I, DN, T, m0, em.m_next)
        assert got.shape == want.shape and got.shape[0] >= 28 * I
        err = np.abs(got - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= TOL, (trial, err)
    return worst


@pytest.mark.parametrize("I,DN,T,generic", _cases())
def test_mixing_thread_code_meets_the_definition(oracle, I, DN, T, generic):
    """Every ratio of the product's table and two generic triples at M = 32, random bin subsets in random order, ragged cuts (empty
    calls, calls shorter than DN frames and than T - 1 frames), offsets 1, 2^32 - 1, 2^32 / 8, an odd large one and a slot at 0 among
    them: every output within 2e-5 of the output's maximum of the float64 definition."""
    worst = _run_against_definition(oracle, I, DN, T, generic, 0, INCS, 100 + I + T + int(generic))
    print("carrier offset, emulation vs definition, (%d, %d, %d)%s: worst %.3g of the maximum" % (I, DN, T, " generic" if generic else "", worst))


@pytest.mark.parametrize("I,DN,T,generic", _cases())
def test_mixing_thread_code_at_any_stream_position(oracle, I, DN, T, generic):
    """The same with the stream's absolute frame index started just below 2^32 (the frame counter's low word wraps in mid-run) and just
    below 2^32 / inc (the phase inc n itself wraps in mid-run): the phase is an integer, so nothing degrades."""
    n = 40 * DN + 13
    w1 = _run_against_definition(oracle, I, DN, T, generic, 2 ** 32 - n // 2, INCS, 200 + I + T)
    inc = 48271
    w2 = _run_against_definition(oracle, I, DN, T, generic, 2 ** 32 // inc - n // 3, [inc, ODD_LARGE, 3 * inc, 0, 2 ** 32 - inc], 300 + I + T)
    print("carrier offset, emulation vs definition at the wraps, (%d, %d, %d)%s: worst %.3g, %.3g of the maximum"
          % (I, DN, T, " generic" if generic else "", w1, w2))


def test_phasor_is_exact_at_zero_and_close_everywhere():
    """phasor_of (resamp_core.hpp): (1, 0) exactly at phase 0 -- the rotation by exactly 1 that test 3 rests on -- and within 2e-7 of
    exp(-j 2 pi ph / 2^32) at the quadrant edges, their neighbours and random phases (float32: 6e-8 per rounding)."""
    from tests.emul import resamp_mix_emul_bind as me
    assert me.phasor(0) == complex(1.0, 0.0)
    rng = np.random.default_rng(5)
    phs = [k * 2 ** 29 + d for k in range(8) for d in (-1, 0, 1)] + [int(v) for v in rng.integers(0, 2 ** 32, 2000)]
    worst = max(abs(me.phasor(p) - np.exp(-2j * np.pi * (p % 2 ** 32) / 2 ** 32)) for p in phs)
    print("phasor_of: worst %.3g" % worst)
    assert worst <= 2e-7, worst


@pytest.mark.parametrize("I,DN,T,generic", _cases())
def test_zero_offsets_through_the_mixing_code_equal_the_picking_code_bit_for_bit(oracle, I, DN, T, generic):
    """All offsets zero: the mixing variant rotates by exactly (1, 0), and equals the picking emulation bit for bit."""
    from tests.emul import resamp_emul_bind as re_
    from tests.emul import resamp_mix_emul_bind as me
    M = 32
    proto = oracle.ResampOracle(M, I, DN, T).h
    rng = np.random.default_rng(400 + I + T + int(generic))
    n = 40 * DN + 13
    x = (rng.standard_normal((n, M)) + 1j * rng.standard_normal((n, M))).astype(np.complex64)
    for trial in range(3):
        cols = rng.permutation(M)[: int(rng.integers(1, M + 1))].astype(np.int32)
        pick = re_.ResampSelectEmul(M, cols, I, DN, T, proto, generic=generic)
        mix = me.ResampMixEmul(M, cols, np.zeros(cols.size, np.uint32), I, DN, T, proto, generic=generic)
        cuts = _cuts(rng, n, DN, T)
        for a, b in zip(cuts, cuts[1:]):
            yp, ym = pick.process(x[a:b]), mix.process(x[a:b])
            assert yp.shape == ym.shape and np.array_equal(yp.view(np.uint32), ym.view(np.uint32)), (trial, a, b)


@pytest.mark.parametrize("I,DN,T,generic", [(18, 25, 16, False), (18, 25, 8, False), (1, 2, 8, False), (5, 7, 11, True)])
def test_offsets_set_in_mid_stream(oracle, I, DN, T, generic):
    """Offsets that change between two calls: from that call on the outputs are, bit for bit, those of an emulation that had the new
    offsets from frame 0 (the delay line is un-rotated, the phase is the absolute frame's); the outputs before are those of the old
    offsets."""
    from tests.emul import resamp_mix_emul_bind as me
    M = 32
    proto = oracle.ResampOracle(M, I, DN, T).h
    rng = np.random.default_rng(500 + I + T)
    n = 40 * DN + 13
    x = (rng.standard_normal((n, M)) + 1j * rng.standard_normal((n, M))).astype(np.complex64)
    cols = rng.permutation(M)[:9].astype(np.int32)
    old = [0, 1, ODD_LARGE, 0, 77, 0, 2 ** 31, 5, 0]
    new = [ODD_LARGE, 1, 0, 0, 2 ** 32 - 77, 123456789, 2 ** 31, 6, 2 ** 29]
    a, b, c = me.ResampMixEmul(M, cols, old, I, DN, T, proto, generic), me.ResampMixEmul(M, cols, old, I, DN, T, proto, generic), \
        me.ResampMixEmul(M, cols, new, I, DN, T, proto, generic)
    cuts = [0, 7, 7 + 3 * DN + 2, 7 + 3 * DN + 2 + (T - 2), 20 * DN, n]
    for k, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
        if k == 2:
            a.set_offsets(new)
        ya, yb, yc = a.process(x[lo:hi]), b.process(x[lo:hi]), c.process(x[lo:hi])
        same_as = yb if k < 2 else yc
        assert np.array_equal(ya.view(np.uint32), same_as.view(np.uint32)), k
        assert ya.shape[0] == 0 or not np.array_equal(ya.view(np.uint32), (yc if k < 2 else yb).view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------------------------- the header


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_carrier_offset_header_symbols_exported_and_bound(pkg):
    """tests/test_abi.py's rule for include/ext/tetra_carrier_offset.h: every function it declares is exported by the library and bound
    with as many parameters in wbrx_binding.CARRIER_OFFSET_ABI; the header compiles as C; the pinned headers keep their counts."""
    hdr = os.path.join(ROOT, "include", "ext", "tetra_carrier_offset.h")
    src = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): m.group(2).split(",") for m in re.finditer(r"\b(?:int|uint32_t)\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    table = pkg.wbrx_binding.CARRIER_OFFSET_ABI
    assert len(decls) == 3 and set(decls) == set(table)
    L = pkg.wbrx_binding._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        assert len(table[name][1]) == len(params) == len(fn.argtypes), name
    assert L.tetra_wbrx_carrier_offset_from_hz.restype is C.c_uint32 and table["tetra_wbrx_carrier_offset_from_hz"][1][:2] == [C.c_double, C.c_double]
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    s = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tetra_wbrx.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(tetra_wbrx_[a-z0-9_]+)\s*\(", s))) == 14
    assert "tetra_wbrx_bin_power is\n * taken in front of the mixer" in open(hdr).read()


def test_carrier_offset_from_hz(pkg):
    """inc = round(f D / Fs 2^32) mod 2^32 by tetra_chan_shift_from_hz's rules: +-6250 Hz at Fs 800 kHz and D 16 is an eighth of a turn
    per frame either way; a negative offset wraps; a non-finite offset or a rate <= 0 gives 0."""
    f = pkg.wbrx_binding.carrier_offset_from_hz
    assert f(6250.0, 800e3, 16) == 2 ** 32 // 8
    assert f(-6250.0, 800e3, 16) == 2 ** 32 - 2 ** 32 // 8
    assert f(0.0, 800e3, 16) == 0 and f(50000.0, 800e3, 16) == 0              # a whole turn per frame wraps to none
    assert f(100.0, 20e6, 400) == round(100.0 * 400 / 20e6 * 2 ** 32)
    assert (f(-100.0, 20e6, 400) + f(100.0, 20e6, 400)) % 2 ** 32 == 0
    assert f(1000.0, 20e6, 400) == pkg.chan_binding.shift_from_hz(1000.0 * 400, 20e6)
    for bad in ((float("nan"), 800e3, 16), (float("inf"), 800e3, 16), (6250.0, 0.0, 16), (6250.0, -1.0, 16), (6250.0, 800e3, 0)):
        assert f(*bad) == 0, bad


def test_carrier_offset_entry_points_refuse_bad_handles_and_lists(pkg):
    """A NULL handle or a NULL list is an argument error; on a machine without a GPU no handle exists (create returns
    TETRA_ERR_NO_DEVICE) and the setter and the getter say the same whatever they are given."""
    L = pkg.wbrx_binding._lib()
    inc = (C.c_uint32 * 4)(1, 2, 3, 4)
    want = ERR_ARG if _has_gpu() else ERR_NO_DEVICE
    assert L.tetra_wbrx_set_carrier_offsets(None, inc, None) == want
    assert L.tetra_wbrx_set_carrier_offsets(None, None, None) == want
    assert L.tetra_wbrx_get_carrier_offsets(None, inc) == want
    assert L.tetra_wbrx_get_carrier_offsets(None, None) == want
    assert list(inc) == [1, 2, 3, 4]
    if not _has_gpu():
        with pytest.raises(pkg.TetraDemodError) as e:
            pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, offsets_hz=[0.0, 6250.0, -6250.0])
        assert e.value.status == ERR_NO_DEVICE
