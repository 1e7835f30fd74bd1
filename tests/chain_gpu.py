"""One way to drive a receive-chain handle (pkg.RxChain) from the GPU tests: the row tuple its rows are compared as, its own bits read
where they lie, a stream in overlapping calls with the results fetched one call late, and a stream in blocking calls with hooks."""
import numpy as np


def device_bytes(torch, ptr, shape, typestr):
    import tetra_amd
    return torch.as_tensor(tetra_amd.pkg.wbrx_binding._DeviceArray(ptr, shape, typestr), device="cuda")


def bit_rows(torch, rx, n_ch):
    """the demodulated bits of the handle's latest call, per channel, as bytes"""
    p, stride, pn = rx.bits_device(0, torch.cuda.current_stream())
    nb = device_bytes(torch, pn, (n_ch,), "<i4").cpu().numpy()
    bits = device_bytes(torch, p, (n_ch, stride), "|u1").cpu().numpy()
    return [bits[c, : nb[c]].tobytes() for c in range(n_ch)]


def rows(blocks, type1):
    """(channel, bitnum, crc_ok, time on entry, time, type-1 bytes) per row (frame_slot counts frames within one call, so it is left out)"""
    return [(int(b["channel"]), int(b["bitnum"]), int(b["crc_ok"]), int(b["tdma_time_rx"]), int(b["tdma_time"]), type1[j].tobytes())
            for j, b in enumerate(blocks)]


def collect(rx, R, which=0):
    return {k: rows(*rx.fetch(k, which)) for k in range(R.N_KINDS)}


def ragged_cuts(n):
    cuts, sizes, i = [0], (9000, 180, 1, 0, 4000), 0
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + sizes[i % len(sizes)]))
        i += 1
    return cuts


def enqueue(torch, rx, d_iq, a, b, s):
    """samples [a, b) of the device array d_iq [C][N] as the handle's next call on stream s, behind the current stream's work"""
    chunk = d_iq[:, a:b].contiguous() if b > a else d_iq[:, :1].contiguous()
    s.wait_stream(torch.cuda.current_stream(d_iq.device))
    rx.process_device(chunk, b - a, s)
    chunk.record_stream(s)


def run_stream(pkg, iq, cuts, flags=0, max_samples=16000, between=None):
    """the stream through one handle, call k = samples [cuts[k], cuts[k+1]), results fetched one call late -> {kind: rows in call order};
    between(rx, k, s) runs after call k is enqueued"""
    import torch
    R = pkg.rx_binding
    dev = torch.device("cuda", 0)
    d_iq = torch.from_numpy(iq).to(dev)
    rx = pkg.RxChain(iq.shape[0], max_samples, flags=flags)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    got = {k: [] for k in range(R.N_KINDS)}
    for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
        enqueue(torch, rx, d_iq, a, b, s)
        if i >= 1:
            for k, v in collect(rx, R, which=1).items():
                got[k] += v
        if between:
            between(rx, i, s)
    for k, v in collect(rx, R, which=0).items():
        got[k] += v
    rx.wait()
    rx.close()
    return got


def run_calls(pkg, iq, cuts, flags, per_call, setup=None, after=None):
    """The stream in blocking calls through one handle on the current stream, call k = samples [cuts[k], cuts[k+1]): setup(rx) before the
    first, per_call(rx, k, stream) behind each, after(rx) behind the last -> (the chain's own bits per channel, the cells, after's value)"""
    import torch
    dev = torch.device("cuda", 0)
    d_iq = torch.from_numpy(np.array(iq)).to(dev)
    n_ch = iq.shape[0]
    rx = pkg.RxChain(n_ch, max(b - a for a, b in zip(cuts, cuts[1:])), flags=flags)
    s = torch.cuda.current_stream(dev)
    bits, extra = [b""] * n_ch, None
    try:
        if setup:
            setup(rx)
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            rx.process_device(d_iq[:, a:b].contiguous(), b - a, s)
            per_call(rx, i, s)
            bits = [x + y for x, y in zip(bits, bit_rows(torch, rx, n_ch))]
        cells = [bytes(c) for c in rx.cells()]
        if after:
            extra = after(rx)
        rx.wait()
    finally:
        rx.close()
    return [np.frombuffer(b, np.uint8) for b in bits], cells, extra
