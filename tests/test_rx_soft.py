"""The receive chain's soft-decision option (TETRA_RX_FLAG_SOFT, include/tetra_rx.h; lane code csrc/soft_core.hpp).

CPU: the lane code built for the host (tests/emul/lmac_soft_emul.cpp) against the reference's own soft decoder -- sign-descramble ->
block_deinterleave -> depuncture onto zeros -> conv_cch_decode -> crc16_ccitt_bits (oracle/_ref) -- bit for bit, the quantiser against a
numpy binary32 restatement, and the operating point of the GPU gain test from the reference-only host pipeline (tests/soft_pipeline.py),
whose rows are the fixture tests/golden/rx_soft_golden.npz.
GPU: the chain with the flag equals that fixture row for row, however the stream is cut, on two streams and on one, through a ring of
minimum size, beside the AACH's Reed-Muller option, through the wideband handle and the one-step delivery, and across a channel reset."""
import os

import numpy as np
import pytest

from tests import chain_host as ch
from tests import soft_pipeline as sp
from tests.chain_gpu import collect, ragged_cuts, run_stream
from tests.chain_host import OP_CHANNELS, OP_SAMPLES, OP_SCHF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ch.RX_SOFT_GOLDEN
OP_ESN0_DB = 11.0                                            # tests/chain_host.py's operating point at the level DESIGN.md 8.3 chose
KINDS = ("sb1", "sb2", "ndb1", "ndb2", "schf")
REF_TPSAP, soft_rows_for = sp.REF_TPSAP, sp.soft_rows_for


@pytest.fixture(scope="module")
def lref(ref):
    if not ref.lmac_available():
        pytest.skip("oracle/_ref/libtetra_lmac_ref.so not available")
    return ref


@pytest.fixture(scope="module")
def semul():
    from tests.emul import lmac_soft_emul_bind
    lmac_soft_emul_bind.build()
    return lmac_soft_emul_bind


# ---- CPU: the lane code against the reference's soft decoder -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_emulated_soft_decoder_equals_the_reference_chain(lref, semul, kind):
    rng = np.random.default_rng(100 + KINDS.index(kind))
    rows, codes = soft_rows_for(lref, kind, rng)
    assert semul.Q() == sp.Q and semul.G() == float(sp.G)
    got_t2, got_ok = semul.decode_rows(kind, rows, None if kind == "sb1" else codes)
    good = 0
    for j in range(len(rows)):
        t2, ok = sp.ref_soft_decode(lref, REF_TPSAP[kind], rows[j], codes[j])
        assert np.array_equal(got_t2[j], t2) and got_ok[j] == ok, (kind, j)
        good += ok
    assert 12 <= good < len(rows)                          # the clean codewords decode, junk does not


def test_emulated_soft_decoder_reads_the_ring_at_any_bit_number(lref, semul):
    """the same row at every alignment of its frame in the ring, wrap included, decodes the same"""
    rng = np.random.default_rng(7)
    rows, codes = soft_rows_for(lref, "schf", rng)
    row, code = rows[1:2], codes[1:2]
    want = sp.ref_soft_decode(lref, 5, row[0], code[0])
    for bn in list(range(0, 8)) + [510, 1024 - 14 - 3, 1024 - 282 - 1, 0xffffffff, 0xfffffe03]:
        t2, ok = semul.decode_rows("schf", row, code, bitnum=[bn])
        assert np.array_equal(t2[0], want[0]) and ok[0] == want[1], bn


def test_quantiser_equals_numpy_float32_and_reproduces_hard_bits(synth, semul):
    assert semul.fresh_prev() == sp.FRESH_PREV.real == sp.FRESH_PREV.imag
    rng = np.random.default_rng(3)
    z = (rng.normal(0, 1, 4000) + 1j * rng.normal(0, 1, 4000)).astype(np.complex64) * rng.choice([1e-3, 0.3, 1, 1, 1.5, 40], 4000).astype(np.float32)
    q, prev = semul.quantise(z)
    assert np.array_equal(q, sp.quantise_np(z)) and prev == z[-1] and q.min() == -sp.Q and q.max() == sp.Q
    q2, _ = semul.quantise(z[1000:], prev=z[999])          # the carried symbol
    assert np.array_equal(q2, q[2000:])
    # noiseless synth symbols, turned back by pi/4 per symbol as the Costas loop leaves them (on the diagonals): the sign is the hard
    # bit (positive <=> 0) for every bit after the first symbol
    tx = synth.hash_bits(5, 6000)
    k = np.arange(3000)
    zs = (synth.bits_to_symbols(tx) * np.exp(-1j * np.pi / 4 * k)).astype(np.complex64)
    qs, _ = semul.quantise(zs)
    assert (np.abs(qs[2:]) >= 15).all() and np.array_equal(qs[2:] < 0, tx[2:] != 0) and np.array_equal(qs, sp.quantise_np(zs))
    # NaN / Inf: a NaN anywhere in the sum gives 0, an infinite sum (from an infinite symbol, or by overflow) +-Q
    inf, nan, one = np.float32(np.inf), np.float32(np.nan), np.complex64(1 + 1j)
    for sym, want in ((complex(nan, 1), [0, 0]), (complex(inf, 1), [0, sp.Q]), (complex(1, inf), [sp.Q, 0]), (complex(-inf, 1), [0, -sp.Q]),
                      (complex(3e38, 3e38), [sp.Q, sp.Q]), (complex(-3e38, -3e38), [-sp.Q, -sp.Q])):
        z1 = np.array([sym], np.complex64)
        qo, _ = semul.quantise(z1, prev=one)
        assert list(qo) == want == list(sp.quantise_np(z1, prev=one)), sym


def test_ring_size_covers_the_synchronisers_buffer_and_two_calls(semul):
    for stride in (8, 1072, 2048, 2049, 6144, 6145, 37920, 1 << 20):
        r = semul.ring_size(stride)
        assert r & (r - 1) == 0 and r >= max(8192, 4096 + 2 * stride) and (r == 8192 or r // 2 < 4096 + 2 * stride)


def test_operating_point_reference_pipeline_gains_and_matches_the_fixture(lref, oracle, synth):
    """The reference-only host pipeline on the GPU gain test's stream: hard decisions leave a clear share of the SCH/F blocks CRC-bad,
    soft decisions recover strictly more; the rows are the committed fixture."""
    iq = ch.operating_point(synth, OP_ESN0_DB)[2]
    for name, use_soft in (("hard", False), ("soft", True)):
        rows = sp.stream_rows(lref, oracle, iq, use_soft)
        schf = rows[ch.KIND_SCH_F]
        assert (len(schf), sum(r[2] for r in schf)) == OP_SCHF[name]
        assert rows == ch.golden_rows(GOLDEN, name)
    assert OP_SCHF["hard"][1] < 0.9 * OP_SCHF["hard"][0] and OP_SCHF["soft"][1] > OP_SCHF["hard"][1]


def test_flag_value_and_binding(pkg):
    src = open(os.path.join(ROOT, "include", "tetra_rx.h")).read()
    assert "TETRA_RX_FLAG_SOFT = 8" in src and pkg.rx_binding.FLAG_SOFT == 8


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def op_iq(synth):
    return ch.operating_point(synth, OP_ESN0_DB)[2]


@pytest.mark.gpu
def test_gpu_flag_8_creates_a_chain(pkg):
    R = pkg.rx_binding
    for flags in (R.FLAG_SOFT, R.FLAG_SOFT | R.FLAG_ONE_STREAM, R.FLAG_SOFT | R.FLAG_AACH_RM3014, R.FLAG_SOFT | 3):
        rx = pkg.RxChain(2, 2000, flags=flags)
        assert rx.count(R.KIND_SCH_F) == 0
        rx.close()
    for flags in (4, 8 | 4, 16, 8 | 16):
        with pytest.raises(pkg.TetraDemodError) as e:
            pkg.RxChain(2, 2000, flags=flags)
        assert e.value.status == -1


@pytest.mark.gpu
@pytest.mark.parametrize("one_stream", [False, True])
def test_gpu_soft_chain_equals_the_host_pipeline(pkg, op_iq, one_stream):
    """row for row: type-1 bits, crc_ok, bitnum, both TDMA times, every kind; the second cut as 9000, 180, 1, 0, 4000, ... samples"""
    R = pkg.rx_binding
    want = ch.golden_rows(GOLDEN, "soft")
    got = run_stream(pkg, op_iq, ragged_cuts(OP_SAMPLES), flags=R.FLAG_SOFT | (R.FLAG_ONE_STREAM if one_stream else 0))
    for k in range(R.N_KINDS):
        assert sorted(got[k]) == sorted(want[k]), (k, len(got[k]), len(want[k]))
    assert len(want[R.KIND_SCH_F]) == OP_SCHF["soft"][0]


@pytest.mark.gpu
def test_gpu_soft_ring_of_minimum_size_wraps(pkg, op_iq, semul):
    """max_samples small enough for the minimum ring (8192 values a channel): one second of bits wraps it four times"""
    R = pkg.rx_binding
    small = 1900
    assert semul.ring_size(pkg.binding.bits_stride(small)) == 8192 and semul.ring_size(pkg.binding.bits_stride(16000)) > 8192
    cuts = list(range(0, OP_SAMPLES, small)) + [OP_SAMPLES]
    a = run_stream(pkg, op_iq, cuts, flags=R.FLAG_SOFT, max_samples=small)
    b = run_stream(pkg, op_iq, [0, 16000, 32000, OP_SAMPLES], flags=R.FLAG_SOFT, max_samples=16000)
    want = ch.golden_rows(GOLDEN, "soft")
    for k in range(R.N_KINDS):
        assert sorted(a[k]) == sorted(b[k]) == sorted(want[k]), k


@pytest.mark.gpu
def test_gpu_soft_recovers_more_blocks_than_hard(pkg, op_iq):
    R = pkg.rx_binding
    cuts = [0, 16000, 32000, OP_SAMPLES]
    hard, soft = run_stream(pkg, op_iq, cuts, flags=0), run_stream(pkg, op_iq, cuts, flags=R.FLAG_SOFT)
    want = ch.golden_rows(GOLDEN, "hard")
    for k in range(R.N_KINDS):
        assert sorted(hard[k]) == sorted(want[k]), k          # the flag-off chain: the hard path's host walk, as ever
    n = {name: sum(r[2] for r in rows[R.KIND_SCH_F]) for name, rows in (("hard", hard), ("soft", soft))}
    print("SCH/F blocks with a good CRC of %d: hard %d, soft %d" % (len(hard[R.KIND_SCH_F]), n["hard"], n["soft"]))
    assert n["soft"] > n["hard"] and (n["hard"], n["soft"]) == (OP_SCHF["hard"][1], OP_SCHF["soft"][1])


@pytest.mark.gpu
def test_gpu_soft_beside_the_aach_option_and_through_the_delivery(pkg, op_iq):
    from tests.emul import rm3014_emul_bind
    R = pkg.rx_binding
    want = ch.golden_rows(GOLDEN, "soft")
    rx = pkg.RxChain(OP_CHANNELS, OP_SAMPLES, flags=R.FLAG_SOFT | R.FLAG_AACH_RM3014)
    rx.process(op_iq)
    rx.wait()
    got = collect(rx, R)
    for k in range(R.N_KINDS):
        if k != R.KIND_BBK:
            assert got[k] == want[k], k
    # the AACH: the pass-through rows of the soft run (descrambled under ITS codes) through the Reed-Muller decoder
    words = np.array([int("".join(str(b) for b in r[5]), 2) for r in want[R.KIND_BBK]], np.uint32)
    cw, dist = rm3014_emul_bind.decode(words)
    exp = [r[:2] + (int(d <= 3),) + r[3:5] + (bytes((int(w) >> (29 - i)) & 1 for i in range(30)),) for r, w, d in zip(want[R.KIND_BBK], cw, dist)]
    assert got[R.KIND_BBK] == exp and np.array_equal(rx.fetch_aach_dist(), dist)
    # the one-step delivery with TETRA_RX_OUT_CRC_GOOD: exactly the rows of every kind whose CRC is good
    dl = rx.deliver(crc_good_only=True).wait()
    for k in range(R.N_KINDS):
        blocks, t1 = rx.fetch(k)
        keep = blocks["crc_ok"] != 0
        assert np.array_equal(dl[k][0], blocks[keep]) and np.array_equal(dl[k][1][:, :t1.shape[1]], t1[keep]), k
    assert 0 < (rx.fetch(R.KIND_SCH_F)[0]["crc_ok"] != 0).sum() == OP_SCHF["soft"][1]
    rx.close()


@pytest.mark.gpu
def test_gpu_soft_through_the_wideband_handle(pkg, synth):
    """32 bins, 3 carriers at 25 dB: the wideband handle carries the flag to its chain -- same frames as the hard handle, and every block
    the hard decoder passes the soft decoder passes with the same bits"""
    import torch
    from tests.test_wbrx import _capture, _rows
    R = pkg.rx_binding
    x, cells, tx = _capture(torch, synth, 32, {1: 11, 7: 12, 20: 13}, 40)
    runs = {}
    for flags in (0, R.FLAG_SOFT):
        wb = pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=x.shape[0], flags=flags)
        wb.process_device(x)
        runs[flags] = _rows(wb.rx, R)
        wb.close()
    hard, soft = runs[0], runs[R.FLAG_SOFT]
    for k in range(R.N_KINDS):
        assert [r[:2] for r in hard[k]] == [r[:2] for r in soft[k]] and len(hard[k]) >= (8 if k != R.KIND_BBK else 30), k
        if k != R.KIND_BBK:
            both = [(h, s) for h, s in zip(hard[k], soft[k]) if h[2]]
            assert len(both) >= 5 and all(s[2] == 1 and s[5] == h[5] for h, s in both), k
    with pytest.raises(pkg.TetraDemodError):
        pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=1 << 16, flags=R.FLAG_SOFT | 4)


@pytest.mark.gpu
def test_gpu_soft_reset_of_one_channel_mid_stream(pkg, op_iq):
    """tetra_rx_reset_channels_device on channel 1 of 3 between two calls: from the next call on that channel is a fresh handle's, bit
    numbering and soft values alike; the others never notice"""
    R = pkg.rx_binding
    iq, step, at = op_iq[:3], 6000, 2
    cuts = list(range(0, OP_SAMPLES + 1, step))

    def between(rx, i, s):
        if i == at - 1:
            rx.reset_channels([1], s)

    got = run_stream(pkg, iq, cuts, flags=R.FLAG_SOFT, max_samples=step, between=between)
    fresh = run_stream(pkg, np.ascontiguousarray(iq[:, at * step:]), cuts[:len(cuts) - at], flags=R.FLAG_SOFT, max_samples=step)
    want = ch.golden_rows(GOLDEN, "soft")
    for k in range(R.N_KINDS):
        for c in (0, 2):
            assert sorted(r for r in got[k] if r[0] == c) == sorted(r for r in want[k] if r[0] == c), (k, c)
        # channel 1: the rows of the first `at` calls are the untouched run's (bit numbers below those calls' bits), then a fresh handle's
        mine, fr = [r for r in got[k] if r[0] == 1], [r for r in fresh[k] if r[0] == 1]
        assert len(fr) >= 3 and mine[len(mine) - len(fr):] == fr, k
        head = mine[:len(mine) - len(fr)]
        assert head == [r for r in want[k] if r[0] == 1][:len(head)], k
