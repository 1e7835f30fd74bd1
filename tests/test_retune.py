"""Retuning while the stream runs (include/tetra_retune.h): tetra_wbrx_retune moves carrier slots of a wideband receiver to other
bins, tetra_rx_reset_channels_device restarts single channels of a receive chain -- both enqueued, neither touching the rest.

Every claim is held bit for bit against code that exists without the feature: a handle that is never retuned (kept slots), the
channeliser -> full resampler composition on all bins (a moved slot's IQ), a separate receive chain reset at the retune point (a
moved slot's blocks and state).  The per-channel resets and the history ring are also run on the host, lane by lane."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.restart_gpu import assert_exported_and_bound, chain_snap as _chain_snap, drive, has_gpu as _has_gpu, frames_i32 as _frames_i32, snap as _snap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_UNSUPPORTED, ERR_NO_DEVICE = -1, -2, -3


# ---------------------------------------------------------------------------------------------------------------------- CPU


def test_retune_header_symbols_all_exported_and_bound(pkg):
    assert_exported_and_bound(pkg, "tetra_retune.h", pkg.rx_binding.RX_RETUNE_EXPORTS + pkg.wbrx_binding.WBRX_RETUNE_EXPORTS,
                              (("tetra_wbrx.h", "tetra_wbrx_", 14), ("tetra_rx.h", "tetra_rx_", len(pkg.rx_binding.RX_EXPORTS))))          # the pinned headers did not grow
    assert callable(pkg.WidebandRx.retune) and callable(pkg.WidebandRx.retune_count) and callable(pkg.RxChain.reset_channels)


def test_retune_entry_points_without_a_gpu_return_no_device(pkg):
    """No handle exists on a machine without a GPU (create returns TETRA_ERR_NO_DEVICE), and every entry point of the header says
    the same whatever it is given; with a GPU a NULL handle is an argument error."""
    pkg.rx_binding._lib()
    L = pkg.wbrx_binding._lib()
    bins = (C.c_int32 * 4)(1, 2, 3, 4)
    a, b = C.c_int64(7), C.c_int64(7)
    want = ERR_ARG if _has_gpu() else ERR_NO_DEVICE
    assert L.tetra_rx_reset_channels_device(None, bins, 4, None) == want
    assert L.tetra_rx_reset_channels_device(None, None, 0, None) == want
    assert L.tetra_wbrx_retune(None, bins, None) == want
    assert L.tetra_wbrx_retune(None, None, None) == want
    assert L.tetra_wbrx_retune_count(None, C.byref(a), C.byref(b)) == want
    assert (a.value, b.value) == (7, 7)
    if not _has_gpu():
        with pytest.raises(pkg.TetraDemodError) as e:
            pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16)
        assert e.value.status == ERR_NO_DEVICE


N_HIST, N_FAR, N_YBUF, N_QRING, N_CD = 80, 48, 7, 4096, 1024          # tetra_demod.h: the per-channel arrays' lengths
POISON_F, POISON_I = np.float32(np.nan), np.int32(0x7A7A7A7A)


def _poisoned_demod(em, Cn, taps, fresh, tr_omega):
    f = {n: np.full(Cn, POISON_F, np.float32) for n in ("agc_g", "fll_ph", "fll_fr", "mu", "omega", "cph", "cfr", "ph2", "q_err")}
    i = {n: np.full(Cn, POISON_I, np.int32) for n in ("offset", "prev", "rrc_valid", "q_ptr", "q_disp", "q_sync", "cd_fill", "cd_blocks")}
    big = {"hist": 2 * N_HIST, "hist_far": 2 * N_FAR, "ybuf": 2 * N_YBUF, "q_ring": N_QRING, "cd_blk": 2 * N_CD}
    f.update({n: np.full((Cn, w), POISON_F, np.float32) for n, w in big.items()})
    arrays = dict(f, **i)
    v = em.DemodView()
    tap_fields = ("q_ring", "q_ptr", "q_disp", "q_sync", "q_err", "cd_blk", "cd_fill", "cd_blocks")
    for name, ctype in em.DemodView._fields_:
        if name in arrays and (taps or name not in tap_fields):
            setattr(v, name, arrays[name].ctypes.data_as(ctype))
    v.n_hist, v.n_hist_far, v.n_ybuf, v.n_q_ring, v.n_cd, v.rrc_all = N_HIST, N_FAR, N_YBUF, N_QRING, N_CD, 128
    v.tr_omega, v.fresh = tr_omega, int(fresh)
    return v, arrays


@pytest.mark.parametrize("taps", [False, True])
@pytest.mark.parametrize("lanes", [64, 1, 7])
def test_reset_lane_code_leaves_a_poisoned_channel_as_create_does(taps, lanes):
    """csrc/retune_core.hpp on the host: every per-channel field of a poisoned demodulator, synchroniser and cell state reads, after the
    reset of the listed channels, what tetra_demod_create / tetra_bsync_create / tetra_rx_create leave (tetra_demod.hip reset_range
    with fresh: gain 1, omega the design's, rrc_valid 128, everything else 0; all-zero State, bit buffer and cell), field by field;
    the channels not listed keep every poisoned byte.  Under the quirks rule only what PI4DQPSK::reset touches changes."""
    from tests.emul import retune_emul_bind as em
    L = em.lib()
    Cn, chans = 9, np.array([7, 0, 4], np.int32)
    others = [c for c in range(Cn) if c not in chans]
    tr_omega = np.float32(2.0)
    fresh_value = {"agc_g": 1.0, "omega": tr_omega, "rrc_valid": 128}
    touched_by_quirks = ("agc_g", "fll_ph", "fll_fr", "rrc_valid", "mu", "omega", "offset", "cph", "cfr")
    tap_fields = ("q_ring", "q_ptr", "q_disp", "q_sync", "q_err", "cd_blk", "cd_fill", "cd_blocks")
    for fresh in (True, False):
        v, arr = _poisoned_demod(em, Cn, taps, fresh, tr_omega)
        before = {n: a.copy() for n, a in arr.items()}
        L.retune_emul_reset_demod(C.byref(v), chans.ctypes.data, chans.size, lanes)
        for n, a in arr.items():
            assert np.array_equal(a[others].view(np.uint32), before[n][others].view(np.uint32)), (n, "another channel was written")
            written = (n in touched_by_quirks) if not fresh else (taps or n not in tap_fields)
            if not written:
                assert np.array_equal(a[chans].view(np.uint32), before[n][chans].view(np.uint32)), (n, fresh)
                continue
            want = fresh_value.get(n, 0)
            if not fresh and n == "rrc_valid":
                want = 0                       # the reference's FIR::reset: the RRC sees none of the shared delay line
            assert np.array_equal(a[chans], np.full_like(a[chans], want)), (n, fresh)
            assert not np.signbit(a[chans].astype(np.float64)).any(), n           # +0, never -0
    # synchroniser (State: 4 words, bit buffer 4096 bytes) and cell state (10 words)
    state = np.full((Cn, 4), 0x7A7A7A7A, np.uint32)
    carry = np.full((Cn, 1024), 0x7A7A7A7A, np.uint32)
    cell = np.full((Cn, 10), 0x7A7A7A7A, np.uint32)
    L.retune_emul_reset_tail(state.ctypes.data, 4, carry.ctypes.data, 1024, cell.ctypes.data, 10, chans.ctypes.data, chans.size, lanes)
    for a in (state, carry, cell):
        assert not a[chans].any() and (a[others] == 0x7A7A7A7A).all()


@pytest.mark.parametrize("M,T", [(32, 16), (800, 16), (12, 2), (5, 9)])
def test_history_ring_on_the_host_rebuilds_the_delay_line_for_any_cut(M, T):
    """keep_element / rebuild_element on the host: after any sequence of calls (empty ones, one frame, fewer than T - 1, many) the
    rebuilt delay-line columns of arbitrary (slot, bin) pairs are the T - 1 newest frames of those bins, zeros before the stream's
    start, and the columns not listed keep their content."""
    from tests.emul import retune_emul_bind as em
    L = em.lib()
    hist = T - 1
    rng = np.random.default_rng(M * 100 + T)
    n = 9 * T + 5
    x = (rng.standard_normal((n, M)) + 1j * rng.standard_normal((n, M))).astype(np.complex64)
    ring = np.full((hist, M), np.nan + 0j, np.complex64)
    cuts = [0, 0, 1, 2, 2, 2 + hist - 1, 2 + 2 * hist, 2 + 2 * hist + 1, 5 * T, 5 * T + hist, n]
    Cn = min(M, 6)
    for a, b in zip(cuts, cuts[1:]):
        part = np.ascontiguousarray(x[a:b]) if b > a else np.zeros((1, M), np.complex64)
        L.retune_emul_keep(part.ctypes.data, M, a, b - a, hist, ring.ctypes.data)
        slots = rng.permutation(Cn)[: int(rng.integers(1, Cn + 1))].astype(np.int32)
        bins = rng.permutation(M)[: slots.size].astype(np.int32)
        line = np.full((hist, Cn), 7 + 7j, np.complex64)
        L.retune_emul_rebuild(ring.ctypes.data, M, hist, b, slots.ctypes.data, bins.ctypes.data, slots.size, Cn, line.ctypes.data)
        want = np.concatenate([np.zeros((hist, M), np.complex64), x[:b]])[-hist:]
        assert np.array_equal(np.ascontiguousarray(line[:, slots]).view(np.uint32), np.ascontiguousarray(want[:, bins]).view(np.uint32)), (a, b)
        rest = [c for c in range(Cn) if c not in slots]
        assert (line[:, rest] == 7 + 7j).all()


# ---------------------------------------------------------------------------------------------------------------------- GPU
#
# Config-5 geometry (M 800, D 400, 20 MHz): ONE cs16 capture with 16 coded downlinks (tests/test_wbrx.py's generator: each carrier
# its own cell -- MCC, MNC, colour code), 40 slots = 0.567 s, cut into ragged blocks; S = 4 slots.

BINS16 = [3 + 53 * i for i in range(15)] + [797]
CARRIERS16 = {k: 31 + i for i, k in enumerate(BINS16)}
NSLOTS = 40
T_RES = 16                                   # the resampler's taps per phase: T - 1 = 15 delay-line frames
D = 400


@pytest.fixture(scope="module")
def band(pkg, synth):
    import torch
    from tests.wideband_gpu import capture, cs16
    x, cells, tx = capture(torch, synth, 800, CARRIERS16, NSLOTS)
    xs = cs16(torch, x)
    del x
    torch.cuda.empty_cache()
    return xs, cells


def _ragged(L, seed, sizes=(150, 399, 400, 401, 9000, 250000, 777777, 1500000)):
    rng = np.random.default_rng(seed)
    cuts = [0]
    while cuts[-1] < L:
        cuts.append(min(L, cuts[-1] + int(rng.choice(sizes))))
    return cuts


def _run(pkg, torch, wb, xs, cuts, retunes):
    """Feed the cuts, retune before call i where retunes has i; -> per call the per-slot snapshots."""
    return drive(pkg, torch, wb, xs, list(zip(cuts, cuts[1:])), {i: (lambda w, bins=bins: w.retune(bins)) for i, bins in retunes.items()})[0]


def _good_sb1(snap_slot, pkg):
    return [r for r in snap_slot["rows"][pkg.rx_binding.KIND_SB1] if r[2]]


@pytest.mark.gpu
def test_gpu_kept_slots_are_untouched_and_an_identical_list_is_a_no_op(pkg, band):
    """Handle A is never retuned, handle B is retuned five times in slots 2 and 3 (to carriers, to noise bins, swapped), handle N gets
    the identical list before every call.  Slots 0 and 1 of B and all slots of N: every call's resampled frames, every kind's rows,
    labels and type-1 bits, cell, sync and demodulator state equal A's as byte patterns."""
    import torch
    xs, _ = band
    L = xs.shape[0]
    cuts = _ragged(L, 5)
    assert len(cuts) > 12
    bins = [BINS16[0], BINS16[15], BINS16[5], BINS16[9]]
    mk = lambda: pkg.WidebandRx(bins, max_in=1500000)
    A, B, N = mk(), mk(), mk()
    plan = {2: bins[:2] + [BINS16[7], BINS16[9]], 3: bins[:2] + [400, 401], 5: bins[:2] + [401, 400], 8: bins[:2] + [BINS16[9], BINS16[7]],
            len(cuts) - 3: bins}
    ra = _run(pkg, torch, A, xs, cuts, {})
    rb = _run(pkg, torch, B, xs, cuts, plan)
    rn = _run(pkg, torch, N, xs, cuts, {i: bins for i in range(len(cuts) - 1)})
    for i, (sa, sb, sn) in enumerate(zip(ra, rb, rn)):
        for c in (0, 1):
            assert sb[c] == sa[c], (i, c)
        assert sn == sa, i
    assert any(_good_sb1(s[0], pkg) for s in ra) and any(_good_sb1(s[1], pkg) for s in ra)          # (the comparison saw locked receivers)
    moved, cur = 0, bins
    for i in sorted(plan):
        moved += sum(x != y for x, y in zip(cur, plan[i]))
        cur = plan[i]
    assert list(B.bins()) == bins and B.retune_count() == (5, moved) and moved >= 8
    assert N.retune_count() == (len(cuts) - 1, 0) and A.retune_count() == (0, 0)
    for h in (A, B, N):
        h.close()


@pytest.mark.gpu
def test_gpu_retuned_slot_iq_is_the_full_resamplers_column_from_the_first_frame(pkg, band):
    """After each retune, every slot's frames of every later call equal column bins[slot] of Channeliser(800) -> Resampler(800) on the
    same capture and cuts, as u32 patterns, first frame included.  The calls before the retunes bring 0, 1, 14 and >= 15 channeliser
    frames, and calls shorter than D follow them; a full-width handle (bins 0 .. M - 1, the in-place resampler) is retuned too."""
    import torch
    xs, _ = band
    L = xs.shape[0]
    #        call: 0       1 (0 fr)  2 (1 fr)  3 (0)   4 (25 fr)  5 (0)    6 (14 fr)         7         8 (0 fr) 9
    cuts = [0, 300000, 300100, 300700, 300705, 310705, 310710, 310710 + 14 * D, 1000003, 1000010, min(L, 2500000)]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    bins0 = [BINS16[1], BINS16[2], 500, BINS16[15]]
    plan = {2: [BINS16[1], BINS16[3], 500, BINS16[15]], 3: [BINS16[1], BINS16[3], 0, 799], 4: [BINS16[4], BINS16[3], 0, 799],
            5: [BINS16[4], BINS16[3], 799, 0], 7: [BINS16[6], 1, 2, 3], 9: [BINS16[1], BINS16[2], 500, BINS16[15]]}
    want_before = {2: 0, 3: 1, 4: 0, 5: 25, 7: 14, 9: 0}
    wb = pkg.WidebandRx(bins0, max_in=max_in)
    full = pkg.WidebandRx(list(range(800)), max_in=max_in, kinds=1)
    full_plan = {3: [1, 0] + list(range(2, 800)), 7: [1, 0] + list(range(2, 798)) + [799, 798]}
    ch = pkg.Channeliser(800, decimation=D, max_in=max_in)
    rs = pkg.Resampler(800, max_in=(D - 1 + max_in) // D)
    chan_buf = torch.zeros(((D - 1 + max_in) // D, 800), dtype=torch.complex64, device="cuda")
    res_buf = torch.zeros((((D - 1 + max_in) // D) * 18 // 25 + 1, 800), dtype=torch.complex64, device="cuda")
    s = torch.cuda.current_stream()
    cur, cur_full, nf_prev, total = list(bins0), list(range(800)), None, 0
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        if i in plan:
            assert nf_prev == want_before[i], (i, nf_prev)
            wb.retune(plan[i], s)
            cur = plan[i]
            assert list(wb.bins()) == cur
        if i in full_plan:
            full.retune(full_plan[i], s)
            cur_full = full_plan[i]
        part = xs[a:b]
        wb.process_device(part, b - a, s)
        full.process_device(part, b - a, s)
        nf_prev = ch.process_device(part, b - a, chan_buf, s)
        nr = rs.process_device(chan_buf, nf_prev, res_buf, s)
        total += nr
        ref = torch.view_as_real(res_buf[:nr]).contiguous().view(torch.int32).cpu().numpy()          # [nr][800][2]
        got = _frames_i32(torch, wb)
        assert got.shape[0] == nr
        for c, k in enumerate(cur):
            assert np.array_equal(got[:, c], ref[:, k]), (i, c, k)
        gf = _frames_i32(torch, full)
        assert np.array_equal(gf, ref[:, cur_full]), i
    assert total == -(-(cuts[-1] // D) * 18 // 25) and total > 4000 and wb.retune_count()[0] == 6
    wb.close(), full.close()


def _reference_chain(pkg, torch, S, max_samples, demod_flags, flags=0):
    return pkg.RxChain(S, max_samples, layout=pkg.binding.LAYOUT_TIME_MAJOR, demod_flags=demod_flags, flags=flags)


def _feed_chain(torch, rx, wb, dummy):
    """The wideband handle's latest frames into a plain chain."""
    p, n = wb.frames_device(0, torch.cuda.current_stream())
    rx.process_device(p if n else dummy.data_ptr(), n, torch.cuda.current_stream())


@pytest.mark.gpu
@pytest.mark.parametrize("quirks", [False, True])
def test_gpu_retuned_slot_chain_equals_a_chain_reset_at_the_retune_point(pkg, band, quirks):
    """Slot 2 moves to another carrier before call 2, and slots 0 and 1 swap (a moved bin is fresh in both indices) before call 4; both
    calls are shorter than D.  Per retune point a separate tetra_rx handle is fed the wideband handle's own frames call for call and
    reset (tetra_rx_reset) at that point: from there to the end of the capture the moved slots' rows, labels (bit numbers from 0),
    type-1 bits, cell, sync and demodulator state equal that chain's channel, call for call -- with and without
    TETRA_FLAG_REFERENCE_QUIRKS (under which every reset keeps the delay line).  At the end every slot reads its carrier's cell."""
    import torch
    xs, cells = band
    L = xs.shape[0]
    cuts = [0, 100000, 200001, 200301, 400000, 400399] + list(range(1900000, L, 1500000)) + [L]
    max_in = max(b - a for a, b in zip(cuts, cuts[1:]))
    fl = pkg.binding.FLAG_REFERENCE_QUIRKS if quirks else 0
    bins = [BINS16[0], BINS16[1], BINS16[2], BINS16[3]]
    wb = pkg.WidebandRx(bins, max_in=max_in, demod_flags=fl)
    dummy = torch.zeros(64, dtype=torch.complex64, device="cuda")
    plan = {2: ([bins[0], bins[1], BINS16[8], bins[3]], [2]), 4: ([bins[1], bins[0], BINS16[8], bins[3]], [0, 1])}
    refs = {i: _reference_chain(pkg, torch, 4, wb.rx.max_samples, fl) for i in plan}
    good = {c: 0 for c in range(4)}
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        if i in plan:
            wb.retune(plan[i][0])
            refs[i].reset()
        wb.process_device(xs[a:b], b - a)
        sw = _chain_snap(pkg, wb.rx, 4)
        for at, rx in refs.items():
            _feed_chain(torch, rx, wb, dummy)
            if i < at:
                continue
            sr = _chain_snap(pkg, rx, 4)
            for c in plan[at][1]:
                assert sw[c] == sr[c], (i, at, c)
                good[c] += len(_good_sb1(sw[c], pkg))
                if i == at:          # bit numbering restarted: no label beyond what this one call can hold (one bit per sample)
                    assert all(r[1] <= wb.frames_device(0)[1] for rows in sw[c]["rows"].values() for r in rows), (i, c)
    assert all(good[c] >= 1 for c in (0, 1, 2)), good          # (the moved receivers locked: the comparison saw decoded blocks)
    cell = wb.rx.cells()
    for c, k in enumerate(plan[4][0]):
        assert (cell[c].mcc, cell[c].mnc, cell[c].colour_code) == cells[k], (c, k)
    assert wb.retune_count() == (2, 3)
    wb.close()
    for rx in refs.values():
        rx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("one_stream", [False, True])
def test_gpu_retune_with_calls_in_flight(pkg, band, one_stream):
    """process, retune, process, retune, process on a side stream with no wait anywhere (two calls in flight; the two-stream chain and
    TETRA_RX_FLAG_ONE_STREAM) leaves the latest and the previous call's results, frames and all state equal to the same sequence with
    tetra_rx_wait before and after every retune.  And a call's results fetched after a retune are what they were before it."""
    import torch
    xs, _ = band
    L = xs.shape[0]
    cuts = [0, 5000000, 6500000, 6500200, 8000000, L]          # slot 3 is never moved: it is locked when the last call runs
    bins = [BINS16[0], BINS16[1], BINS16[2], BINS16[3]]
    plan = {1: [BINS16[4], BINS16[1], BINS16[2], BINS16[3]], 2: [BINS16[4], BINS16[1], BINS16[5], BINS16[3]],
            3: [BINS16[4], BINS16[7], BINS16[5], BINS16[3]], 4: [BINS16[0], BINS16[7], BINS16[6], BINS16[3]]}
    fl = pkg.rx_binding.FLAG_ONE_STREAM if one_stream else 0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fast = pkg.WidebandRx(bins, max_in=5000000, flags=fl)
    slow = pkg.WidebandRx(bins, max_in=5000000, flags=fl)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        if i in plan:
            fast.retune(plan[i], side)
        fast.process_device(xs[a:b], b - a, side)
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        if i in plan:
            slow.rx.wait()
            before = _snap(pkg, torch, slow) if i == 3 else None
            slow.retune(plan[i], side)
            slow.rx.wait()
            if before is not None:          # the previous call's results, fetched after the retune: unchanged
                after = _snap(pkg, torch, slow)
                for c in range(4):
                    assert after[c]["rows"] == before[c]["rows"] and after[c]["frames"] == before[c]["frames"], c
                    if c == 1:                   # the slot this retune moves: its state is fresh, the others' is not touched
                        assert after[c]["sync"] == (0, 0, 0, 0) and after[c]["cell"] == bytes(40)
                    else:
                        assert (after[c]["sync"], after[c]["cell"], after[c]["demod"]) == (before[c]["sync"], before[c]["cell"], before[c]["demod"])
        slow.process_device(xs[a:b], b - a, side)
    with torch.cuda.stream(side):
        for which in (0, 1):
            assert _snap(pkg, torch, fast, which) == _snap(pkg, torch, slow, which), which
    assert _good_sb1(_snap(pkg, torch, fast)[3], pkg)          # (the comparison saw decoded blocks)
    fast.rx.wait()
    fast.close(), slow.close()


@pytest.mark.gpu
def test_gpu_retune_refuses_bad_lists_and_changes_nothing(pkg, band):
    """A duplicate bin, a bin outside [0, M) and a NULL list are TETRA_ERR_ARG; the bin list and all later output equal those of a
    handle that never saw the calls."""
    import torch
    xs, _ = band
    cuts = [0, 1000000, 2000000, 3000000]
    bins = [BINS16[0], BINS16[1], BINS16[2], BINS16[3]]
    A, B = pkg.WidebandRx(bins, max_in=1000000), pkg.WidebandRx(bins, max_in=1000000)
    ra = _run(pkg, torch, A, xs, cuts, {})
    rb = []
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        for bad in ([bins[0], bins[1], bins[2], bins[0]], [bins[0], 800, bins[2], bins[3]], [-1, bins[1], bins[2], bins[3]]):
            with pytest.raises(pkg.TetraDemodError) as e:
                B.retune(bad)
            assert e.value.status == ERR_ARG
        assert pkg.wbrx_binding._lib().tetra_wbrx_retune(B._h, None, None) == ERR_ARG
        with pytest.raises(ValueError):
            B.retune(bins[:3])
        assert list(B.bins()) == bins
        B.process_device(xs[a:b], b - a)
        rb.append(_snap(pkg, torch, B))
    assert ra == rb and B.retune_count() == (0, 0)
    with pytest.raises(TypeError):
        B.rx.reset_channels([0])
    one = (C.c_int32 * 1)(0)          # the C entry point refuses a wideband handle's chain too
    assert pkg.rx_binding._lib().tetra_rx_reset_channels_device(B.rx._h, one, 1, None) == ERR_UNSUPPORTED
    B.process_device(xs[:1000000], 1000000)
    A.process_device(xs[:1000000], 1000000)
    assert _snap(pkg, torch, A) == _snap(pkg, torch, B)
    A.close(), B.close()


@pytest.mark.gpu
def test_gpu_walking_one_slot_across_the_band(pkg, band):
    """Slot 1 is stepped across all 16 carriers, one pass of the capture (0.567 s, ragged blocks) on each; slots 0, 2 and 3 stay.  A
    16-slot handle that is never retuned sees the same stream.  On every stop the reference handle has CRC-good SB1 blocks on that
    carrier (checked first), and so has the walking slot; the cell state it reads there is the carrier's own (MCC, MNC, colour code)
    and its scrambling code, and equals the reference handle's cell of that carrier in those fields."""
    import torch
    xs, cells = band
    L = xs.shape[0]
    R = pkg.rx_binding
    fixed = [400, 401, 402]                                   # noise bins: the walking slot is the only receiver
    walk = pkg.WidebandRx([fixed[0], BINS16[0], fixed[1], fixed[2]], max_in=1500000, kinds=1 << R.KIND_SB1)
    ref = pkg.WidebandRx(BINS16, max_in=1500000, kinds=1 << R.KIND_SB1)
    for stop, k in enumerate(BINS16):
        if stop:
            walk.retune([fixed[0], k, fixed[1], fixed[2]])
        cuts = _ragged(L, 100 + stop)
        good_ref = good_walk = 0
        for a, b in zip(cuts, cuts[1:]):
            walk.process_device(xs[a:b], b - a)
            ref.process_device(xs[a:b], b - a)
            bw, _ = walk.rx.fetch(R.KIND_SB1)
            br, _ = ref.rx.fetch(R.KIND_SB1)
            good_walk += int(((bw["channel"] == 1) & (bw["crc_ok"] == 1)).sum())
            good_ref += int(((br["channel"] == stop) & (br["crc_ok"] == 1)).sum())
        assert good_ref >= 1, (stop, k, "the dwell is too short for the reference handle itself")
        assert good_walk >= 1, (stop, k)
        cw, cr = walk.rx.cells()[1], ref.rx.cells()[stop]
        assert (cw.mcc, cw.mnc, cw.colour_code) == cells[k], (stop, k)
        assert cw.scramb_init == pkg.synth.tx_scramb_code(*cells[k])
        assert (cw.mcc, cw.mnc, cw.colour_code, cw.scramb_init) == (cr.mcc, cr.mnc, cr.colour_code, cr.scramb_init)
    assert walk.retune_count() == (15, 15)
    walk.close(), ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("quirks", [False, True])
def test_gpu_rx_reset_channels_on_a_plain_chain(pkg, band, quirks):
    """Plain tetra_rx handles on the same four carriers' frames: X has channels 3 and 1 reset before call 4 (a call shorter than D;
    enqueued, no wait), W is
    reset as a whole there (tetra_rx_reset), Y is created there, Z is never touched.  From call 4 on X's channels 1 and 3 equal W's --
    and Y's, a fresh handle's, unless TETRA_FLAG_REFERENCE_QUIRKS makes every reset keep the delay line -- and its channels 0 and 2
    equal Z's: rows, labels, type-1 bits, cell, sync and demodulator state.  Bad lists are refused and change nothing."""
    import torch
    xs, _ = band
    L = xs.shape[0]
    cuts = [0, 50000, 100000, 150000, 200000, 200250] + list(range(1600000, L, 1400000)) + [L]
    fl = pkg.binding.FLAG_REFERENCE_QUIRKS if quirks else 0
    src = pkg.WidebandRx([BINS16[10], BINS16[11], BINS16[12], BINS16[13]], max_in=max(b - a for a, b in zip(cuts, cuts[1:])), kinds=1)
    ms = src.rx.max_samples
    X, W, Z = (_reference_chain(pkg, torch, 4, ms, fl) for _ in range(3))
    Y = None
    dummy = torch.zeros(64, dtype=torch.complex64, device="cuda")
    lib = pkg.rx_binding._lib()
    good = 0
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        src.process_device(xs[a:b], b - a)
        if i == 4:
            for bad in ([1, 1], [4], [-1], [0, 1, 2, 3, 0]):
                arr = (C.c_int32 * len(bad))(*bad)
                assert lib.tetra_rx_reset_channels_device(X._h, arr, len(bad), None) == ERR_ARG, bad
            assert lib.tetra_rx_reset_channels_device(X._h, None, 2, None) == ERR_ARG
            X.reset_channels([])
            X.reset_channels([3, 1], torch.cuda.current_stream())
            W.reset()
            if not quirks:
                Y = _reference_chain(pkg, torch, 4, ms, fl)
        for h in (X, W, Y, Z):
            if h is not None:
                _feed_chain(torch, h, src, dummy)
        sx, sw, sz = (_chain_snap(pkg, h, 4) for h in (X, W, Z))
        for c in (0, 2) if i >= 4 else (0, 1, 2, 3):
            assert sx[c] == sz[c], (i, c)
        if i >= 4:
            for c in (1, 3):
                assert sx[c] == sw[c], (i, c)
                assert sx[c] != sz[c], (i, c)
                good += len(_good_sb1(sx[c], pkg))
            if Y is not None:
                sy = _chain_snap(pkg, Y, 4)
                for c in (1, 3):
                    assert sx[c] == sy[c], (i, c)
    assert good >= 2          # (both restarted receivers locked again: the comparison saw decoded blocks)
    for h in (X, W, Y, Z, src):
        if h is not None:
            h.close()
