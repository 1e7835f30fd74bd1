"""Off-centre carriers through the ORACLE composition, on the CPU: channeliser oracle -> numpy pre-mix by each carrier's offset ->
resampler oracle -> oracle demodulator -> the reference's receive chain (oracle/_ref), on the known-answer band of
tests/test_carrier_offset_gpu.py (M 32, D 16, 80 slots; carriers 7 and 20 off their bins' centres by +f and -f, 1 and 31 on theirs).
Per channeliser prototype (taps_per_channel, chan_cutoff_rel) and carrier: (CRC-good SCH/F blocks, CRC-bad ones, CRC-bad ones behind
the eighth).  This is where the test's prototype and the counts in its docstring come from.

  python profiles/carrier_offset_composition.py [f_hz]          (default 6250)"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tetra_amd  # noqa: E402
from oracle import binding as ob  # noqa: E402
from oracle import ref_binding as ref  # noqa: E402

synth = tetra_amd.pkg.synth
M, D, NSLOTS = 32, 16, 80
BINS = [1, 7, 20, 31]
CARRIERS = {1: 11, 7: 12, 20: 13, 31: 14}


def capture(off_hz, seed=1, noise=1e-3):
    """tests/test_carrier_offset_gpu.py::_capture_offsets in numpy (its own noise generator)."""
    fs = M * 25000.0
    N = (NSLOTS * 510 - 100) // 9 * 9
    L = int(round(N * fs / 36000.0))
    x = np.zeros(L, np.complex128)
    n = np.arange(L, dtype=np.float64)
    for k, sd in CARRIERS.items():
        cell = (100 + 7 * sd % 900, 1000 + 13 * sd, (5 + 3 * sd) % 64)
        tx = synth.gen_downlink(NSLOTS, sd, cell=cell)
        s = synth.gen_channel(N, sd + 100, bits=tx[0], amp=1.0)[0].astype(np.complex128)
        S = np.fft.fft(s)
        Y = np.zeros(L, np.complex128)
        Y[: N // 2] = S[: N // 2]
        Y[L - (N - N // 2):] = S[N // 2:]
        y = np.fft.ifft(Y) * (L / N)
        kc = k if k < M // 2 else k - M
        x += y * np.exp(2j * math.pi * ((kc + off_hz[k] / 25000.0) / M) * n)
    rng = np.random.default_rng(seed)
    x += noise * (rng.standard_normal(L) + 1j * rng.standard_normal(L))
    x *= 0.25 / np.abs(x).max()
    return x.astype(np.complex64)


def compose(x, off_hz, P, cutoff, mix=True):
    f = ob.ChanOracle(M, P, D, cutoff).process(x, BINS).astype(np.complex128)
    nn = np.arange(f.shape[0], dtype=np.float64)
    for j, k in enumerate(BINS):
        if mix:
            f[:, j] *= np.exp(-2j * math.pi * off_hz[k] * D / (M * 25000.0) * nn)
    y = ob.ResampOracle(len(BINS)).process(f.astype(np.complex64))
    bits, nb = ob.process_batch(np.ascontiguousarray(y.T))[:2]
    out = []
    for c in range(len(BINS)):
        rx = ref.ReferenceRxChain()
        rx.feed(bits[c][:nb[c]])
        ok = [e["crc_ok"] for e in rx.events() if e["lchan"] == ref.TETRA_LC_SCH_F]
        out.append((sum(1 for v in ok if v), sum(1 for v in ok if not v), sum(1 for v in ok[8:] if not v)))
        rx.close()
    return out


if __name__ == "__main__":
    f0 = float(sys.argv[1]) if len(sys.argv) > 1 else 6250.0
    off = {1: 0.0, 7: f0, 20: -f0, 31: 0.0}
    x = capture(off)
    for P in (8, 16):
        for cutoff in (1.5, 1.75, 2.0):
            print("f %g Hz, taps_per_channel %d, chan_cutoff_rel %g, pre-mixed:" % (f0, P, cutoff), compose(x, off, P, cutoff), flush=True)
    print("f %g Hz, taps_per_channel 16, chan_cutoff_rel 2, NOT pre-mixed:" % f0, compose(x, off, 16, 2.0, mix=False), flush=True)
