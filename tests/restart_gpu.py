"""What the tests of the three restarts share (tests/test_retune.py, test_handover.py, test_gap.py): planted bit streams for the host
emulation, the reference clock, the small band of one base station, the snapshot a call leaves in a handle, one call loop over a
wideband handle with a hook in front of chosen calls, one matcher of rows by kind and TDMA time, and the build-and-run of the host
banks' C++ drivers."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np

from tests.chain_gpu import bit_rows, collect, device_bytes
from tests.wideband_gpu import cs16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORM_1, NORM_2, SYNC = 0, 1, 3                     # enum tetra_train_seq
TS = 510
CUTS = (1, 509, 510, 511, 1020, "ragged")
DONOR_CELL = (0x12345677, 5, 262, 1, 1, 7, 3, 2, 9, 3)          # scramb_init, cc, mcc, mnc, tcd tn / fn / mn, phy tn / fn / mn



def has_gpu():
    import torch
    return torch.cuda.is_available()


def header_functions(header, prefix="tetra_"):
    """-> (the functions include/<header> declares under `prefix`, sorted; its text without comments)"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, src))), src


def assert_exported_and_bound(pkg, header, exports, pinned):
    """include/<header> declares the three functions `exports`, the library exports them and the bindings give each argument types and
    an int result; the earlier headers `pinned` ((header, prefix, count)) did not grow.  -> the header's text without comments"""
    names, src = header_functions(header)
    assert names == sorted(exports) and len(names) == 3
    L = pkg.load_library()
    for n in names:
        assert hasattr(L, n), n
    pkg.rx_binding._lib(), pkg.wbrx_binding._lib()
    for n in names:
        assert getattr(L, n).argtypes is not None and getattr(L, n).restype is C.c_int, n
    for hdr, prefix, count in pinned:
        assert len(header_functions(hdr, prefix)[0]) == count, hdr
    return src


# ---------------------------------------------------------------------------------------------------------------------- planted streams


def burst(synth, rng, kind):
    """510 bits of random payload with one training sequence where its burst type has it."""
    b = rng.integers(0, 2, TS, dtype=np.uint8)
    if kind == SYNC:
        b[214:214 + 38] = synth.TRAIN_SYNC
    else:
        b[244:244 + 22] = synth.TRAIN_NORM_2 if kind == NORM_2 else synth.TRAIN_NORM_1
    return b


def count_seqs(synth, bits):
    """Positions at which any of the three sequences stands exactly (a planted stream must hold the planted ones only)."""
    hits = []
    for seq in (synth.TRAIN_NORM_1, synth.TRAIN_NORM_2, synth.TRAIN_SYNC):
        if bits.size < seq.size:
            continue
        w = np.lib.stride_tricks.sliding_window_view(bits, seq.size)
        hits += [int(i) for i in np.nonzero((w == seq).all(axis=1))[0]]
    return sorted(hits)


def filler(synth, rng, n):
    """n random bits that hold none of the training sequences."""
    while True:
        b = rng.integers(0, 2, n, dtype=np.uint8)
        if not count_seqs(synth, b):
            return b


def downlink_bits(synth, rng, n_slots):
    """Slots as the reference's receiver needs them to lock and stay locked: a sync burst every 4th slot, normal bursts between."""
    return np.concatenate([burst(synth, rng, SYNC if s % 4 == 0 else (NORM_2 if s % 2 else NORM_1)) for s in range(n_slots)])


def reference_clock(cases, golden):
    """{(tn, fn, mn, k): the time after k tetra_tdma_time_add_tn(t, 1)} for the ((tn, fn, mn), k) in `cases`, from the reference's own
    function (oracle/_ref) where it is built, else from the recording of exactly that (the JSON file `golden`)."""
    from oracle import ref_binding
    if ref_binding.available():
        from tests.chain_host import TdmaTime, ref_add_tn
        add_tn = ref_add_tn(ref_binding)
        out = {}
        for (tn, fn, mn), k in cases:
            t = TdmaTime(tn=tn, fn=fn, mn=mn)
            for _ in range(k):
                add_tn(C.byref(t), 1)
            out[(tn, fn, mn, k)] = (int(t.tn), int(t.fn), int(t.mn))
        return out
    rec = json.load(open(golden))
    return {tuple(r[:4]): tuple(r[4:]) for r in rec["rows"]}


def slot_index(p):
    """Slot number inside the hyperframe of a packed TDMA time of a downlink that started at (1, 1, 1)."""
    tn, fn, mn = int(p) & 0xff, (int(p) >> 8) & 0xff, (int(p) >> 16) & 0xff
    return (mn - 1) * 72 + (fn - 1) * 4 + (tn - 1)


# ---------------------------------------------------------------------------------------------------------------------- the band
#
# One base station on a small band (M = 32 bins at 800 kHz, as tests/test_wbrx.py's small capture): carrier A the control channel (a SYNC
# burst every 4th slot, synth.gen_downlink), carrier B a traffic carrier of the same cell and frame timing with ONE SYNC burst per
# multiframe (slots 16 and 88; and one more at slot 8, because a receiver locks on the first SYNC burst it sees and decodes the second:
# the witness needs code and clock before the move), carrier C another cell (its own colour code) on the same frame timing.  96 slots = 1.36 s.
# A handle refuses two slots on one bin, so the traffic carrier is on the air twice, on bin B for the witness and on bin B2 for the slot
# that moves: the same bits and timing, each with its own noise.
M_BAND, D_BAND = 32, 16
BIN_A, BIN_B, BIN_B2, BIN_C, BIN_EMPTY = 3, 11, 19, 24, 28
CELL_X, CELL_Y = (262, 1, 5), (262, 1, 41)
N_SLOTS, B_SYNC_SLOTS = 96, (8, 16, 88)
CALL = 200000                                # 0.25 s at 800 kHz; the move is at the first boundary, 17.6 slots: just behind B's SYNC burst


def traffic_downlink(synth, n_slots, seed, cell, sync_slots):
    """synth.gen_downlink's slots (the reference's encoders and burst builders), with SYNC bursts only in sync_slots: the others are
    normal bursts, two logical channels (NDB + NDB) in even slots, one (SCH/F) in odd ones."""
    rng = np.random.default_rng(seed)
    mcc, mnc, cc = cell
    code = synth.tx_scramb_code(mcc, mnc, cc)
    field = lambda v, n: [(v >> (n - 1 - i)) & 1 for i in range(n)]
    slots = np.arange(n_slots)
    s_sync = np.array(sorted(sync_slots))
    rest = np.array([s for s in slots if s not in sync_slots])
    s_ndb, s_schf = rest[rest % 2 == 0], rest[rest % 2 == 1]
    pdu = rng.integers(0, 2, (len(s_sync), 60), dtype=np.uint8)
    for r, s in enumerate(s_sync):
        tn, fn, mn = synth.tdma_time_of_slot(int(s))
        pdu[r, 4:10], pdu[r, 10:12], pdu[r, 12:17], pdu[r, 17:23] = field(cc, 6), field(tn - 1, 2), field(fn, 5), field(mn, 6)
        pdu[r, 31:41], pdu[r, 41:55] = field(mcc, 10), field(mnc, 14)
    enc = lambda kind, n, bits: synth.tx_encode(kind, rng.integers(0, 2, (n, bits), dtype=np.uint8), np.full(n, code, np.uint32))
    sb1 = synth.tx_encode("sb1", pdu, np.full(len(s_sync), code, np.uint32))
    sb2, ndb1, ndb2, schf = enc("sb2", len(s_sync), 124), enc("ndb", len(s_ndb), 124), enc("ndb", len(s_ndb), 124), enc("schf", len(s_schf), 268)
    bb = rng.integers(0, 2, (n_slots, 30), dtype=np.uint8) ^ synth.tx_scramb_seq([code], 30)[0][None, :]
    out = np.zeros((n_slots, TS), np.uint8)
    for r, s in enumerate(s_sync):
        out[s] = synth.tx_sync_burst(sb1[r], bb[s], sb2[r])
    for r, s in enumerate(s_ndb):
        out[s] = synth.tx_norm_burst(ndb1[r], bb[s], ndb2[r], 1)
    for r, s in enumerate(s_schf):
        out[s] = synth.tx_norm_burst(schf[r][:216], bb[s], schf[r][216:], 0)
    return out.reshape(-1)


def band_capture(torch, synth, esn0_db=25.0):
    """-> cs16 capture [L][2] on the GPU (tests/wideband_gpu.py's capture with the three carriers above)."""
    dev = torch.device("cuda")
    fs = M_BAND * 25000.0
    N = (N_SLOTS * TS - 100) // 9 * 9
    L = int(round(N * fs / 36000.0))
    x = torch.zeros(L, dtype=torch.complex128, device=dev)
    n = torch.arange(L, dtype=torch.float64, device=dev)
    traffic = traffic_downlink(synth, N_SLOTS, 22, CELL_X, B_SYNC_SLOTS)
    streams = {BIN_A: synth.gen_downlink(N_SLOTS, 21, cell=CELL_X)[0], BIN_B: traffic, BIN_B2: traffic, BIN_C: synth.gen_downlink(N_SLOTS, 23, cell=CELL_Y)[0]}
    for k, tx in streams.items():
        s = torch.from_numpy(synth.gen_channel(N, 200 + k, bits=tx, amp=1.0, cfo=0.0, tau=0.6, phase0=0.1 * k, esn0_db=esn0_db)[0].astype(np.complex128)).to(dev)
        S = torch.fft.fft(s)
        Y = torch.zeros(L, dtype=torch.complex128, device=dev)
        Y[: N // 2] = S[: N // 2]
        Y[L - (N - N // 2):] = S[N // 2:]
        x += torch.fft.ifft(Y) * (L / N) * torch.polar(torch.ones_like(n), 2.0 * math.pi * k / M_BAND * n)
    x *= 0.25 / float(x.abs().max())
    return cs16(torch, x.to(torch.complex64).contiguous())


def band_calls(L, start=0):
    """The capture from sample `start` on in 0.25 s calls, as (first, end) pairs."""
    return [(a, min(a + CALL, L)) for a in range(start, L, CALL)]


# ---------------------------------------------------------------------------------------------------------------------- snapshots


def demod_states(pkg, rx, n):
    L = pkg.binding.load_library()
    out = []
    for c in range(n):
        st = pkg.binding.ChannelState()
        assert L.tetra_demod_get_state(C.c_void_p(rx.demod_handle()), c, C.byref(st)) == 0
        out.append(bytes(st))
    return out


def chain_snap(pkg, rx, n, which=0):
    """What a call leaves in a chain, per channel: every kind's rows (labels + type-1 bits), cell, sync and demodulator state."""
    rows = collect(rx, pkg.rx_binding, which)
    cells, sync, dem = [bytes(c) for c in rx.cells()], rx.sync_states(), demod_states(pkg, rx, n)
    return [dict(rows={k: [r for r in v if r[0] == c] for k, v in rows.items()}, cell=cells[c], sync=sync[c], demod=dem[c]) for c in range(n)]


def frames_i32(torch, wb, which=0):
    p, n = wb.frames_device(which, torch.cuda.current_stream())
    if n == 0:
        return np.zeros((0, wb.n_bins, 2), np.int32)
    return device_bytes(torch, p, (n, wb.n_bins, 2), "<i4").cpu().numpy().copy()


def snap(pkg, torch, wb, which=0):
    """chain_snap of a wideband handle's chain, with every slot's resampled frames"""
    s = chain_snap(pkg, wb.rx, wb.n_bins, which)
    fr = frames_i32(torch, wb, which)
    for c in range(wb.n_bins):
        s[c]["frames"] = fr[:, c].tobytes()
    return s


def drive(pkg, torch, wb, xs, calls, before=None, stream=None, wait=False, feed=None, bits=False):
    """The call loop of the restart tests: xs[a:b] for (a, b) in `calls` through the wideband handle wb on `stream`.  before = {i: hook}:
    hook(wb) runs in front of call i (a retune, a gap), between two tetra_rx_wait with `wait`.  feed(wb, i, a, b) takes process_device's
    place.  -> (per call the per-slot snapshots, with the call's demodulated bits when asked for; per call the hand-over status); both
    stay empty on a side stream that nobody waits for."""
    snaps, status = [], []
    for i, (a, b) in enumerate(calls):
        hook = (before or {}).get(i)
        if hook:
            if wait:
                wb.rx.wait()
            hook(wb)
            if wait:
                wb.rx.wait()
        if feed:
            feed(wb, i, a, b)
        else:
            wb.process_device(xs[a:b], b - a, stream)
        if stream is None or wait:
            s = snap(pkg, torch, wb)
            if bits:
                for c, row in enumerate(bit_rows(torch, wb.rx, wb.n_bins)):
                    s[c]["bits"] = row
            snaps.append(s)
            status.append(wb.handover_status())
    return snaps, status


def in_flight_and_waited(pkg, torch, run):
    """run(stream, wait) -> (.., .., the handle, ..), a drive() with a restart on its way: once on a side stream with no wait anywhere (two
    calls in flight), once with tetra_rx_wait before and after the restart.  The latest and the previous call's snapshots of the two
    handles are equal.  -> (the first run's result, the second's)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fast, slow = run(side, False), run(side, True)
    with torch.cuda.stream(side):
        for which in (0, 1):
            assert snap(pkg, torch, fast[2], which) == snap(pkg, torch, slow[2], which), which
    return fast, slow


def rows_by_time(per_call, channel=None):
    """per_call: {kind: rows} of one call after the other (a row: (channel, bitnum, crc_ok, tdma_time_rx, tdma_time, type-1 bytes)).
    -> ({key: (crc_ok, tdma_time, type-1 bits)}, [key + value] in delivery order) with key = (channel, kind, tdma_time_rx), or for
    `channel`'s rows alone (kind, tdma_time_rx).  Where every key must be there once, the two have the same length."""
    order = [((k, r[3]) if channel is not None else (r[0], k, r[3])) + (r[2], r[4], r[5])
             for rows in per_call for k, v in sorted(rows.items()) for r in v if channel is None or r[0] == channel]
    return {o[:-3]: o[-3:] for o in order}, order


def blocks_by_time(snaps, slot, first_call=0):
    """rows_by_time of one slot's rows in drive()'s snapshots, over the calls from first_call on, under (kind, tdma_time_rx)"""
    return rows_by_time([s[slot]["rows"] for s in snaps[first_call:]], channel=slot)


def build_and_run_bank_driver(pkg, name, args):
    """tests/host/<name>.cpp, a plain C++ driver of host/tetra_rx_bank.h, built against the library and run -> the finished process"""
    pk = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd")
    pkg.build.build()
    exe = os.path.join(ROOT, "tests", "host", name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(pk, "host"),
                    os.path.join(ROOT, "tests", "host", name + ".cpp"), "-L", pk, "-ltetra_demod_hip", "-Wl,-rpath," + pk, "-o", exe], check=True)
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
