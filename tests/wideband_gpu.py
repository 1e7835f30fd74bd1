"""The wideband GPU tests' signal: coded downlinks on the bins of one capture, and its cs16 form."""
import math

import numpy as np


def capture(torch, synth, M, carriers, nslots, seed=1, noise=1e-3):
    """carriers {bin: seed} at Fs = M x 25 kHz -> (x complex64 [n] on cuda, cells {bin: (mcc, mnc, cc)}, tx {bin: gen_downlink}).
    Per carrier a coded downlink (synth.gen_downlink, its own cell) modulated at 36 ksps (synth.gen_channel), raised to the capture rate
    by band-limited interpolation (zero-padding in frequency, float64), shifted to the centre of its bin; summed over a noise floor."""
    dev = torch.device("cuda")
    fs = M * 25000.0
    N = (nslots * 510 - 100) // 9 * 9             # 36 ksps samples; Fs / 36 kHz = M 25 / 36 is a multiple of 1/9
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
        x += y * torch.polar(torch.ones_like(n), 2.0 * math.pi * kc / M * n)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x += noise * torch.view_as_complex(torch.randn((L, 2), device=dev, generator=g, dtype=torch.float64))
    x *= 0.25 / float(x.abs().max())
    return x.to(torch.complex64).contiguous(), cells, tx


def cs16(torch, x):
    return torch.view_as_real(x).mul(32768.0).round().clamp(-32768, 32767).to(torch.int16).contiguous()
