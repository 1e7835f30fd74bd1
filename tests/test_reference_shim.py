"""The reference's OWN src/dsp/*.cpp, compiled where they lie against stand-in core headers, versus the oracle.

Needs oracle/_ref/libref_shim*.so, which build() compiles from the reference sources (oracle/build_ref.sh); skipped where neither
is there.  The reference's
PI4DQPSK / FLL / COMPLEX_FD / PI4DQPSK_COSTAS / DQPSKSymbolExtractor / BitUnpacker sources include SDR++ core headers
and VOLK, which are NOT under /root/reference; tests/refshim/ holds our own restatement of those primitives
(SURVEY.md Appendix A).  So this is EVIDENCE, NOT A PIN: it shows the reference's per-sample loop code, fed the
primitives as we understand them, makes the bit decisions oracle/tetra_oracle.c makes.  Float results differ by
design (libm cosf/sinf and plain multiply-add sums there; the oracle's own sincos polynomial and fmaf chains here),
so in the oracle's CONTRACT mode symbols are compared with the tolerance SURVEY.md Appendix B.4/B.5 measured for
reduction-order changes: rms <= 3e-3, max <= 3e-2, and ALL bits equal.

The second half of the file (test_exact_*) removes that slack: with the oracle in its REFERENCE-FLOAT mode (libm phasors, two
separate complex band-edge dots, plain `acc += a * b` sums, no fmaf: oracle/tetra_oracle.h) every symbol FLOAT, every bit and
the final loop state of the reference's objects must be reproduced BIT FOR BIT -- any transcription slip in fll.cpp:135-149,
complex_fd.cpp:89-151, pi4dqpsk_costas.cpp:5-28 or pi4dqpsk.cpp:32-140 would show as a differing bit pattern.  What is left
between the two oracle modes is exactly the documented recipe (polynomial sincos, fmaf chains, conjugate-pair FLL sums).
"""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import ref_binding

pytestmark = pytest.mark.skipif(ref_binding.shim_path() is None,
                                reason="oracle/_ref/libref_shim.so not built and the reference sources not present")

RMS_TOL = 3e-3
MAX_TOL = 3e-2


def load_reference_build():
    # built by oracle/build_ref.sh (flags and sources there)
    L = C.CDLL(ref_binding.shim_path())
    L.ref_create.restype = C.c_void_p
    L.ref_create.argtypes = [C.c_double, C.c_double, C.c_int] + [C.c_double] * 7
    L.ref_destroy.argtypes = [C.c_void_p]
    L.ref_process.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_process.restype = C.c_int
    L.ref_set_param.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.ref_set_param.restype = C.c_int
    L.ref_reset.argtypes = [C.c_void_p]
    L.ref_set_rrc_params.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.ref_set_rrc_params.restype = None
    L.ref_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_get_state.restype = None
    return L


@pytest.fixture(scope="module")
def ref():
    return load_reference_build()


class RefChain:
    """The reference's objects, constructed with the oracle's Cfg (main.cpp:78-84 values by default)."""

    def __init__(self, L, cfg):
        self.L = L
        # smallest advance of the timing loop per symbol (complex_fd.cpp:136-143): bounds the symbols one call can emit
        self.step = min(1.0, cfg.samplerate / cfg.symbolrate * (1.0 - cfg.omega_rel_limit) - abs(cfg.mu_gain))
        self.h = L.ref_create(cfg.symbolrate, cfg.samplerate, cfg.rrc_tap_count, cfg.rrc_beta, cfg.agc_rate,
                              cfg.costas_bandwidth, cfg.fll_bandwidth, cfg.omega_gain, cfg.mu_gain, cfg.omega_rel_limit)

    def process(self, iq):
        iq = np.ascontiguousarray(iq, np.complex64)
        n = len(iq)
        cap = int((n + 1) / self.step) + 64               # below one sample per symbol a call emits more symbols than samples
        assert cap <= 1000000                             # (the reference's own stream buffers: STREAM_BUFFER_SIZE)
        sym = np.zeros(cap, np.complex64)
        bits = np.zeros(2 * cap, np.uint8)
        ns = self.L.ref_process(self.h, n, iq.ctypes.data_as(C.c_void_p), sym.ctypes.data_as(C.c_void_p),
                                bits.ctypes.data_as(C.c_void_p))
        assert ns >= 0
        return sym[:ns], bits[: 2 * ns]

    def state(self):
        """Loop state of the reference's objects: dict of np.float32 / int in the oracle State's field names."""
        f = np.zeros(9, np.float32)
        i = np.zeros(2, np.int32)
        self.L.ref_get_state(self.h, f.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p))
        return dict(agc_gain=f[0], fll_phase=f[1], fll_freq=f[2], mu=f[3], omega=f[4], costas_phase=f[5], costas_freq=f[6],
                    ph2=f[7], standarderr=f[8], offset=int(i[0]), prev=int(i[1]))

    def set_param(self, pid, v):
        assert self.L.ref_set_param(self.h, pid, float(v)) == 0

    def set_rrc_params(self, taps, beta):
        self.L.ref_set_rrc_params(self.h, int(taps), float(beta))

    def reset(self):
        self.L.ref_reset(self.h)

    def close(self):
        self.L.ref_destroy(self.h)


def _compare(sym_r, bits_r, o):
    assert len(sym_r) == len(o["sym"]) and len(bits_r) == len(o["bits"])
    d = np.abs(sym_r - o["sym"])
    rms = float(np.sqrt((d ** 2).mean())) if len(d) else 0.0
    mx = float(d.max()) if len(d) else 0.0
    nbad = int((bits_r != o["bits"]).sum())
    return rms, mx, nbad


def test_probe_scenario_bits_equal(ref, oracle, synth):
    """SURVEY.md Appendix B.2's scenario: 40060 samples -> 20031 symbols -> 40062 bits, every bit equal."""
    iq, txb, _ = synth.gen_channel(40060, 7, cfo=0.03, tau=5 / 16.0, amp=0.2, esn0_db=25.0)
    r = RefChain(ref, oracle.default_cfg())
    sym, bits = r.process(iq)
    r.close()
    o = oracle.Oracle().process(iq)
    assert len(sym) == 20031 and len(bits) == 40062
    rms, mx, nbad = _compare(sym, bits, o)
    assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (rms, mx, nbad)
    lag, err, n = synth.align_and_count_errors(bits, txb, skip=len(bits) // 2)
    assert err == 0 and n > 19000   # and both are the transmitted bits


@pytest.mark.parametrize("seed", [1234, 1235, 1240, 1299])
def test_baseline_synth_bits_equal(ref, oracle, synth, seed):
    """Channels of the BASELINE workload's generator (random offset / timing / level, 25 dB), one second each."""
    iq, _, _ = synth.gen_channel(36000, seed)
    r = RefChain(ref, oracle.default_cfg())
    sym, bits = r.process(iq)
    r.close()
    o = oracle.Oracle().process(iq)
    rms, mx, nbad = _compare(sym, bits, o)
    assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (rms, mx, nbad)


def test_chunked_streaming_matches(ref, oracle, synth):
    """Carried state across calls (FIR histories, COMPLEX_FD's offset and delay buffer): chunks of 7 / 180 / 4001."""
    iq, _, _ = synth.gen_channel(24000, 42, cfo=-0.02, tau=1.3, amp=0.5)
    whole = oracle.Oracle().process(iq)
    for chunk in (7, 180, 4001):
        r = RefChain(ref, oracle.default_cfg())
        parts = [r.process(iq[i:i + chunk]) for i in range(0, len(iq), chunk)]
        r.close()
        sym = np.concatenate([p[0] for p in parts])
        bits = np.concatenate([p[1] for p in parts])
        rms, mx, nbad = _compare(sym, bits, whole)
        assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (chunk, rms, mx, nbad)


def test_reference_reset_and_setters_to_the_letter(ref, oracle, synth):
    """The quirks switch (TETRA_FLAG_REFERENCE_QUIRKS; oracle: quirks=True / reset_reference) against the reference's own
    reset() and setters: reset() keeps ph2, COMPLEX_FD's delay buffer and the slicer's previous symbol
    (pi4dqpsk.cpp:120-130) and clears the RRC's delay line but NOT the FLL's band-edge FIRs' (rrc.reset() :125 versus
    FLL::reset fll.cpp:120-127 -- this test is what found that; the oracle models it with rrc_valid);
    setRRCBeta(int) truncates (pi4dqpsk.cpp:72-74); loop setters touch only their constants."""
    iq, _, _ = synth.gen_channel(30000, 77, cfo=0.01, tau=0.4, amp=0.3)
    a, b, c = iq[:9001], iq[9001:20000], iq[20000:]
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle()
    outs_r, outs_o = [], []
    outs_r.append(r.process(a)); outs_o.append(o.process(a))
    r.reset(); o.reset_reference()
    outs_r.append(r.process(b)); outs_o.append(o.process(b))
    for pid, v in ((4, 0.03), (5, 0.004), (6, 0.008), (7, 2e-4), (8, 0.02), (9, 0.02)):
        r.set_param(pid, v); o.set_param(pid, v, quirks=True)
    outs_r.append(r.process(c)); outs_o.append(o.process(c))
    for (sym, bits), oo in zip(outs_r, outs_o):
        rms, mx, nbad = _compare(sym, bits, oo)
        assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (rms, mx, nbad)
    # setRRCBeta(int) truncates 0.35 to 0: both sides now run a beta = 0 root-raised cosine (a sinc); nothing locks any
    # more, so compare the first symbols only -- they show the SAME new filter was designed on both sides
    r.set_param(3, 0.35); o.set_param(3, 0.35, quirks=True)
    sym, _ = r.process(iq[:400])
    oo = o.process(iq[:400])
    r.close()
    assert len(sym) == len(oo["sym"]) and np.abs(sym[:40] - oo["sym"][:40]).max() <= MAX_TOL
    o2 = oracle.Oracle()
    o2.process(a); o2.reset_reference(); o2.process(b)
    for pid, v in ((4, 0.03), (5, 0.004), (6, 0.008), (7, 2e-4), (8, 0.02), (9, 0.02)):
        o2.set_param(pid, v, quirks=True)
    o2.process(c)
    o2.set_param(3, 0.35, quirks=False)            # the same call WITHOUT the quirk keeps beta = 0.35: a different filter
    assert np.abs(o2.process(iq[:400])["sym"][:40] - sym[:40]).max() > MAX_TOL


def test_reference_tap_count_setter_mid_stream(ref, oracle, synth):
    """setRRCTapCount mid-stream (pi4dqpsk.cpp:56-70): only the RRC is re-designed, the FLL keeps its 65-tap band-edge
    filters; FIR::setTaps keeps the newest history and zero-fills what a longer filter newly looks back at (as restated
    in tests/refshim/dsp/filter/fir.h).  Shrink to 33, grow to 49 after only 20 samples, then back to 65."""
    iq, _, _ = synth.gen_channel(20000, 78, cfo=-0.015, tau=1.1, amp=0.6)
    cuts = [0, 5000, 5020, 9000, 20000]
    taps = [None, 33, 49, 65]
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle()
    for k in range(4):
        if taps[k]:
            r.set_param(2, taps[k]); o.set_param(2, taps[k], quirks=True)
            assert o.ntaps == taps[k] and int(o.tab.ntaps_be) == 65
        blk = iq[cuts[k]:cuts[k + 1]]
        sym, bits = r.process(blk)
        rms, mx, nbad = _compare(sym, bits, o.process(blk))
        assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (k, rms, mx, nbad)
    r.close()


def test_set_rrc_params_keeps_the_double_roll_off(ref, oracle, synth):
    """setRRCParams(int, double) (pi4dqpsk.cpp:56-66) keeps the roll-off as given -- only setRRCBeta(int)
    truncates.  setRRCParams(49, 0.35) mid-stream on the reference's code versus the oracle's tap count (quirks: RRC only)
    + untruncated roll-off: the stream stays locked and every bit is equal; the truncating form gives another filter."""
    iq, _, _ = synth.gen_channel(14000, 79, cfo=0.012, tau=0.9, amp=0.4)
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle()
    r.process(iq[:7000]); o.process(iq[:7000])
    r.set_rrc_params(49, 0.35)
    o.set_param(2, 49, quirks=True); o.set_param(3, 0.35, quirks=False)
    sym, bits = r.process(iq[7000:])
    r.close()
    oo = o.process(iq[7000:])
    rms, mx, nbad = _compare(sym, bits, oo)
    assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (rms, mx, nbad)
    o2 = oracle.Oracle()
    o2.process(iq[:7000])
    o2.set_param(2, 49, quirks=True); o2.set_param(3, 0.35, quirks=True)       # setRRCBeta(int): roll-off 0
    assert np.abs(o2.process(iq[7000:])["sym"][:200] - sym[:200]).max() > MAX_TOL


def test_other_sample_rate_and_several_chains(ref, oracle, synth):
    """50 ksps (BASELINE config 5's rate: sps 2.78 -- FLL::createBandedgeFilters fll.cpp:61-95 and COMPLEX_FD::init
    complex_fd.cpp:12-28 with sps != 2) and eight chains side by side: reference code versus oracle."""
    cfg = oracle.default_cfg()
    cfg.samplerate = 50000.0
    iq, _, _ = synth.gen_channel(30000, 321, sps=50000.0 / 18000.0, cfo=0.015)
    r = RefChain(ref, cfg)
    sym, bits = r.process(iq)
    r.close()
    rms, mx, nbad = _compare(sym, bits, oracle.Oracle(cfg).process(iq))
    assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (rms, mx, nbad)
    for c in range(8):
        x, _, _ = synth.gen_channel(7000, 900 + c)
        r = RefChain(ref, oracle.default_cfg())
        sym, bits = r.process(x)
        r.close()
        rms, mx, nbad = _compare(sym, bits, oracle.Oracle().process(x))
        assert nbad == 0 and rms <= RMS_TOL and mx <= MAX_TOL, (c, rms, mx, nbad)


# ---------------------------------------------------------------------------------------------------------------------
# Bit-exact: the oracle's reference-float mode against the reference's objects (symbol floats, bits, final loop state)
# ---------------------------------------------------------------------------------------------------------------------
STATE_FLOATS = ("agc_gain", "fll_phase", "fll_freq", "mu", "omega", "costas_phase", "costas_freq", "ph2", "standarderr")
STATE_INTS = ("offset", "prev")


def state_bits(st):
    """A loop state (RefChain.state() dict or an oracle State) as comparable bit patterns."""
    get = (lambda k: st[k]) if isinstance(st, dict) else (lambda k: getattr(st, k))
    return ([int(np.float32(get(k)).view(np.uint32)) for k in STATE_FLOATS], [int(get(k)) for k in STATE_INTS])


def _exact(r, o, sym, bits, oo, what=""):
    assert len(sym) == len(oo["sym"]) and len(bits) == len(oo["bits"]), what
    assert np.array_equal(bits, oo["bits"]), what
    bad = np.flatnonzero((sym.view(np.uint32) != oo["sym"].view(np.uint32)).reshape(-1, 2).any(axis=1))
    assert bad.size == 0, (what, "first differing symbol", int(bad[0]), sym[bad[0]], oo["sym"][bad[0]])
    assert state_bits(r.state()) == state_bits(o.st), (what, r.state(), {k: getattr(o.st, k) for k in STATE_FLOATS + STATE_INTS})


def test_exact_probe_and_baseline_channels(ref, oracle, synth):
    """One call each: the survey's probe scenario and channels of the BASELINE generator (36000 samples)."""
    cases = [synth.gen_channel(40060, 7, cfo=0.03, tau=5 / 16.0, amp=0.2, esn0_db=25.0)[0]]
    cases += [synth.gen_channel(36000, seed)[0] for seed in (1234, 1235, 1240, 1299, 77)]
    for k, iq in enumerate(cases):
        r = RefChain(ref, oracle.default_cfg())
        o = oracle.Oracle(reference_floats=True)
        sym, bits = r.process(iq)
        _exact(r, o, sym, bits, o.process(iq), "case %d" % k)
        r.close()


def test_exact_with_the_float_pi_header_variant(oracle, synth):
    """The same exactness when the reference is compiled against the header variant that spells pi as the float macro FL_M_PI
    (-DREFSHIM_FLOAT_PI; tests/refshim/dsp/processor.h): its objects then design OTHER tables (58 of 65 RRC taps, 849 of 1024
    interpolator taps differ), and the oracle's reference-float mode handed those tables -- read out of the reference's objects --
    reproduces every symbol float, bit and the loop state bit for bit: the per-sample transcription does not lean on the tables,
    and the tables are data."""
    L = C.CDLL(ref_binding.shim_path(float_pi=True))
    L.ref_create.restype = C.c_void_p
    L.ref_create.argtypes = [C.c_double, C.c_double, C.c_int] + [C.c_double] * 7
    L.ref_destroy.argtypes = [C.c_void_p]
    L.ref_process.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_process.restype = C.c_int
    L.ref_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.ref_get_state.restype = None
    L.ref_get_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 4 + [C.POINTER(C.c_int)]
    L.ref_get_tables.restype = C.c_int
    changed = 0
    for seed in (1234, 1240, 77):
        iq, _, _ = synth.gen_channel(24000, seed)
        r = RefChain(L, oracle.default_cfg())
        rrc, re, im, bank = (np.zeros(n, np.float32) for n in (129, 129, 129, 1024))
        nb = C.c_int(0)
        n = L.ref_get_tables(r.h, *(a.ctypes.data_as(C.c_void_p) for a in (rrc, re, im, bank)), C.byref(nb))
        o = oracle.Oracle(reference_floats=True)
        assert n == o.ntaps == 65 and nb.value == 65
        changed = int((rrc[:65].view(np.uint32) != o.rrc_taps().view(np.uint32)).sum())
        for i in range(65):
            o.tab.rrc[i], o.tab.be_a[i], o.tab.be_b[i] = float(rrc[i]), float(re[i]), float(im[i])
        for p in range(128):
            for k in range(8):
                o.tab.bank[p][k] = float(bank[8 * p + k])
        for a, b in ((0, 9001), (9001, 9008), (9008, 24000)):
            sym, bits = r.process(iq[a:b])
            _exact(r, o, sym, bits, o.process(iq[a:b]), "seed %d [%d, %d)" % (seed, a, b))
        r.close()
    assert changed >= 50          # (58: really other tables than the double-pi design)


def test_exact_chunked_streaming(ref, oracle, synth):
    """Carried state call after call (7 / 180 / 4001 samples): exact after EVERY call, not only at the end."""
    iq, _, _ = synth.gen_channel(12000, 42, cfo=-0.02, tau=1.3, amp=0.5)
    for chunk in (7, 180, 4001):
        r = RefChain(ref, oracle.default_cfg())
        o = oracle.Oracle(reference_floats=True)
        for i in range(0, len(iq), chunk):
            sym, bits = r.process(iq[i:i + chunk])
            _exact(r, o, sym, bits, o.process(iq[i:i + chunk]), "chunk %d at %d" % (chunk, i))
        r.close()


def test_exact_reset_and_setters(ref, oracle, synth):
    """reset() and every loop setter mid-stream, then setRRCBeta(int)'s truncation (pi4dqpsk.cpp:72-74, pi4dqpsk.h:56)."""
    iq, _, _ = synth.gen_channel(30000, 77, cfo=0.01, tau=0.4, amp=0.3)
    a, b, c = iq[:9001], iq[9001:20000], iq[20000:]
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle(reference_floats=True)
    sym, bits = r.process(a); _exact(r, o, sym, bits, o.process(a), "before reset")
    r.reset(); o.reset_reference()
    assert state_bits(r.state()) == state_bits(o.st)
    sym, bits = r.process(b); _exact(r, o, sym, bits, o.process(b), "after reset")
    for pid, v in ((4, 0.03), (5, 0.004), (6, 0.008), (7, 2e-4), (8, 0.02), (9, 0.02)):
        r.set_param(pid, v); o.set_param(pid, v, quirks=True)
    sym, bits = r.process(c); _exact(r, o, sym, bits, o.process(c), "after the loop setters")
    r.set_param(3, 0.35); o.set_param(3, 0.35, quirks=True)
    sym, bits = r.process(iq[:4000]); _exact(r, o, sym, bits, o.process(iq[:4000]), "after setRRCBeta(int)")
    r.close()


def test_exact_tap_count_setters_and_set_rrc_params(ref, oracle, synth):
    """setRRCTapCount shrinking / growing / growing again mid-stream (FIR::setTaps' history rule, rrc_valid) and
    setRRCParams(49, 0.35) (the double roll-off survives)."""
    iq, _, _ = synth.gen_channel(20000, 78, cfo=-0.015, tau=1.1, amp=0.6)
    cuts = [0, 5000, 5020, 9000, 20000]
    taps = [None, 33, 49, 65]
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle(reference_floats=True)
    for k in range(4):
        if taps[k]:
            r.set_param(2, taps[k]); o.set_param(2, taps[k], quirks=True)
        blk = iq[cuts[k]:cuts[k + 1]]
        sym, bits = r.process(blk)
        _exact(r, o, sym, bits, o.process(blk), "tap count step %d" % k)
    r.close()
    iq, _, _ = synth.gen_channel(14000, 79, cfo=0.012, tau=0.9, amp=0.4)
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle(reference_floats=True)
    sym, bits = r.process(iq[:7000]); _exact(r, o, sym, bits, o.process(iq[:7000]), "before setRRCParams")
    r.set_rrc_params(49, 0.35)
    o.set_param(2, 49, quirks=True); o.set_param(3, 0.35, quirks=False)
    sym, bits = r.process(iq[7000:]); _exact(r, o, sym, bits, o.process(iq[7000:]), "after setRRCParams")
    r.close()


def test_exact_other_rates_and_rate_setters(ref, oracle, synth):
    """50 ksps at create (config 5's rate), then setSamplerate / setSymbolrate mid-stream (pi4dqpsk.cpp:32-54: RRC re-designed,
    timing loop reset by COMPLEX_FD::setOmega, band-edge filters untouched)."""
    cfg = oracle.default_cfg()
    cfg.samplerate = 50000.0
    iq, _, _ = synth.gen_channel(30000, 321, sps=50000.0 / 18000.0, cfo=0.015)
    r = RefChain(ref, cfg)
    o = oracle.Oracle(cfg, reference_floats=True)
    sym, bits = r.process(iq[:20000]); _exact(r, o, sym, bits, o.process(iq[:20000]), "50 ksps")
    r.set_param(1, 48000.0); o.set_param(1, 48000.0, quirks=True)
    sym, bits = r.process(iq[20000:26000]); _exact(r, o, sym, bits, o.process(iq[20000:26000]), "after setSamplerate")
    r.set_param(0, 17000.0); o.set_param(0, 17000.0, quirks=True)
    sym, bits = r.process(iq[26000:]); _exact(r, o, sym, bits, o.process(iq[26000:]), "after setSymbolrate")
    r.close()


def test_exact_below_one_sample_per_symbol_step(ref, oracle, synth):
    """The part of COMPLEX_FD::process's domain where floor(mu) can be 0 -- several symbols from one offset
    (complex_fd.cpp:98-145: `offset += delta` with delta == 0): 1.0 and 0.9 samples per symbol (omega_min - |mu gain| =
    0.96 / 0.86).  Cut into ONE-sample calls on both sides, so a call that returns two symbols IS such an event; the run has
    to contain many.  (At 2 samples per symbol no muGain short of ~2 stalls the loop: the detector's error is a difference
    of neighbouring interpolator rows, a few 1e-2 -- measured, so rates are what reaches this code.)"""
    for rate, seed in ((18000.0, 555), (16200.0, 557)):
        cfg = oracle.default_cfg()
        cfg.samplerate = rate
        iq, _, _ = synth.gen_channel(3000, seed, sps=1.02)
        r = RefChain(ref, cfg)
        o = oracle.Oracle(cfg, reference_floats=True)
        multi = 0
        for i in range(len(iq)):
            sym, bits = r.process(iq[i:i + 1])
            _exact(r, o, sym, bits, o.process(iq[i:i + 1]), "rate %g sample %d" % (rate, i))
            multi += len(sym) >= 2
        r.close()
        assert multi > 50, (rate, multi)
        # and as one call
        r = RefChain(ref, cfg)
        o = oracle.Oracle(cfg, reference_floats=True)
        sym, bits = r.process(iq)
        assert len(sym) > len(iq) * 0.99
        _exact(r, o, sym, bits, o.process(iq), "rate %g, one call" % rate)
        r.close()


def test_exact_long_filters_and_very_slow_timing_loops(ref, oracle, synth):
    """The rest of the domain the product's generic kernel covers: 73 / 100 / 129 taps (PI4DQPSK::init takes any count,
    pi4dqpsk.cpp:11-30) and 0.12 samples per symbol (~8 symbols from every offset), incl. setRRCTapCount(101) mid-stream."""
    for prm, sps in ((dict(rrc_tap_count=73), 2.0), (dict(rrc_tap_count=100), 2.0), (dict(rrc_tap_count=129, rrc_beta=0.3), 2.0),
                     (dict(samplerate=18000.0 * 0.12), 1.02), (dict(samplerate=18000.0 * 0.2, rrc_tap_count=90), 1.02)):
        cfg = oracle.default_cfg()
        for k, v in prm.items():
            setattr(cfg, k, v)
        iq, _, _ = synth.gen_channel(2500, 7100 + len(prm), sps=sps)
        r = RefChain(ref, cfg)
        o = oracle.Oracle(cfg, reference_floats=True)
        for a, b in ((0, 1), (1, 800), (800, 2500)):
            if "samplerate" in prm:          # the reference's stream buffer holds STREAM_BUFFER_SIZE symbols: keep calls short
                b = min(b, a + 600)
            sym, bits = r.process(iq[a:b])
            _exact(r, o, sym, bits, o.process(iq[a:b]), str(prm))
        r.close()
    iq, _, _ = synth.gen_channel(6000, 7200)
    r = RefChain(ref, oracle.default_cfg())
    o = oracle.Oracle(reference_floats=True)
    sym, bits = r.process(iq[:3000]); _exact(r, o, sym, bits, o.process(iq[:3000]), "before growth")
    r.set_param(2, 101); o.set_param(2, 101, quirks=True)
    sym, bits = r.process(iq[3000:]); _exact(r, o, sym, bits, o.process(iq[3000:]), "after setRRCTapCount(101)")
    r.close()
