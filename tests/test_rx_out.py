"""One-step hand-off of a receive-chain call's decoded blocks to the host (include/tetra_rx_out.h): every selected kind gathered by
the GPU into one self-describing buffer (page-locked host memory or device memory), asynchronous, optionally packed and CRC-filtered,
ordered against later calls.  The yardstick is tetra_rx_fetch: a delivery holds exactly its rows."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.chain_gpu import enqueue, rows as _rows
from tests.chain_host import PACKED_BYTES, TYPE1_BITS as TYPE1, downlink_batch as _downlink_batch, noisy_batch as _noisy_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PK = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd")
SAN = os.path.join(ROOT, "tests", "san")


def test_rx_out_header_symbols_all_exported(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tetra_rx_out.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tetra_rx_[a-z0-9_]+)\s*\(", src)))
    L = pkg.load_library()
    assert set(names) == set(pkg.rx_binding.RX_OUT_EXPORTS)
    assert not set(names) & set(pkg.rx_binding.RX_EXPORTS)
    for n in names:
        assert hasattr(L, n), n


def test_rx_out_struct_layouts_match_header(pkg):
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "tetra_rx_out.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %u\\n",'
            ' sizeof(tetra_rx_out_kind_t), sizeof(tetra_rx_out_header_t), offsetof(tetra_rx_out_kind_t, blocks_offset),'
            ' offsetof(tetra_rx_out_kind_t, bits_offset), offsetof(tetra_rx_out_header_t, status), offsetof(tetra_rx_out_header_t, n_kinds),'
            ' offsetof(tetra_rx_out_header_t, call), offsetof(tetra_rx_out_header_t, bytes), offsetof(tetra_rx_out_header_t, kinds),'
            ' TETRA_RX_OUT_PACKED, TETRA_RX_OUT_CRC_GOOD, TETRA_RX_OUT_MAGIC);return 0;}\n')
    with tempfile.TemporaryDirectory() as td:
        cfile = os.path.join(td, "s.c")
        open(cfile, "w").write(prog)
        exe = os.path.join(td, "s")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    R = pkg.rx_binding
    K, H = R.OutKind, R.OutHeader
    assert v == [C.sizeof(K), C.sizeof(H), K.blocks_offset.offset, K.bits_offset.offset, H.status.offset, H.n_kinds.offset,
                 H.call.offset, H.bytes.offset, H.kinds.offset, R.OUT_PACKED, R.OUT_CRC_GOOD, R.OUT_MAGIC]
    assert C.sizeof(H) == 224


def _build_delivery(R, rows, flags, rng):
    """A delivery laid out by hand as include/tetra_rx_out.h documents it: {kind: n_rows} -> (buffer, {kind: (blocks, bits)})."""
    kinds = sorted(rows)
    hd = R.OutHeader()
    hd.magic, hd.status, hd.flags, hd.n_kinds, hd.call = R.OUT_MAGIC, 0, flags, len(kinds), 41
    off, want = C.sizeof(R.OutHeader), {}
    for i, k in enumerate(kinds):
        n = rows[k]
        rb = PACKED_BYTES[k] if flags & R.OUT_PACKED else TYPE1[k]
        e = hd.kinds[i]
        e.kind, e.n_rows, e.n_rows_decoded, e.row_bytes = k, n, n + 2, rb
        e.blocks_offset = (off + 15) // 16 * 16
        e.bits_offset = (e.blocks_offset + 24 * n + 15) // 16 * 16
        off = e.bits_offset + rb * n
        blocks = np.zeros(n, R.BLOCK_DTYPE)
        blocks["channel"], blocks["bitnum"], blocks["crc_ok"] = np.arange(n), 510 * np.arange(n), rng.integers(0, 2, n)
        want[k] = (blocks, rng.integers(0, 256 if flags & R.OUT_PACKED else 2, (n, rb)).astype(np.uint8))
    hd.bytes = off
    buf = np.zeros(off, np.uint8)
    buf[:C.sizeof(R.OutHeader)] = np.frombuffer(bytes(hd), np.uint8)
    for i, k in enumerate(kinds):
        e = hd.kinds[i]
        b, t = want[k]
        buf[e.blocks_offset: e.blocks_offset + 24 * len(b)] = np.frombuffer(b.tobytes(), np.uint8)
        buf[e.bits_offset: e.bits_offset + t.size] = t.reshape(-1)
    return buf, want


def test_rx_out_view_reads_the_documented_layout(pkg):
    R = pkg.rx_binding
    L = pkg.load_library()
    rng = np.random.default_rng(5)
    for flags in (0, R.OUT_PACKED, R.OUT_CRC_GOOD, R.OUT_PACKED | R.OUT_CRC_GOOD):
        rows = {0: 3, 1: 17, 3: 0, 5: 9}
        buf, want = _build_delivery(R, rows, flags, rng)
        hd, got = R.view_delivery(buf)
        assert hd.call == 41 and sorted(got) == sorted(rows)
        for k in rows:
            assert got[k][0].tobytes() == want[k][0].tobytes() and np.array_equal(got[k][1], want[k][1]), (flags, k)
        # a kind the delivery does not hold; truncated and corrupt buffers are statuses
        p = buf.ctypes.data_as(C.c_void_p)
        n = C.c_int(-1)
        assert L.tetra_rx_out_view(p, buf.nbytes, 2, None, None, C.byref(n), None) == -2
        assert L.tetra_rx_out_view(p, buf.nbytes, 6, None, None, None, None) == -1
        for short in (0, 100, 223, 224, buf.nbytes - 1):
            assert L.tetra_rx_out_view(p, short, 5, None, None, None, None) == -1, short
        for field, value in (("magic", 0), ("n_kinds", 7), ("bytes", buf.nbytes + 1), ("flags", 8)):
            bad = buf.copy()
            hd2 = R.OutHeader.from_buffer(bad)
            setattr(hd2, field, value)
            del hd2
            assert L.tetra_rx_out_view(bad.ctypes.data_as(C.c_void_p), bad.nbytes, 5, None, None, None, None) == -1, field
        for field, value in (("n_rows", 10 ** 6), ("blocks_offset", buf.nbytes - 16), ("bits_offset", 8), ("row_bytes", 33)):
            bad = buf.copy()
            hd2 = R.OutHeader.from_buffer(bad)
            setattr(hd2.kinds[3], field, value)         # kind 5's entry
            del hd2
            assert L.tetra_rx_out_view(bad.ctypes.data_as(C.c_void_p), bad.nbytes, 5, None, None, None, None) == -1, field
        bad = buf.copy()
        hd2 = R.OutHeader.from_buffer(bad)
        hd2.status = -6
        del hd2
        assert L.tetra_rx_out_view(bad.ctypes.data_as(C.c_void_p), bad.nbytes, 5, None, None, None, None) == -6


def test_rx_out_unpack_bits_equals_numpy(pkg):
    R = pkg.rx_binding
    L = pkg.load_library()
    rng = np.random.default_rng(6)
    for nbits, rb in list(zip(TYPE1, PACKED_BYTES)) + [(1, 1), (9, 2), (268, 40), (15, 3)]:
        packed = rng.integers(0, 256, (23, rb)).astype(np.uint8)
        got = R.unpack_bits(packed, nbits)
        assert np.array_equal(got, np.unpackbits(packed, axis=1)[:, :nbits]), (nbits, rb)
    out = np.zeros(64, np.uint8)
    packed = np.zeros(8, np.uint8)
    assert L.tetra_rx_unpack_bits(packed.ctypes.data_as(C.c_void_p), 1, 8, 65, out.ctypes.data_as(C.c_void_p), 65) == -1
    assert L.tetra_rx_unpack_bits(packed.ctypes.data_as(C.c_void_p), 1, 8, 60, out.ctypes.data_as(C.c_void_p), 59) == -6
    assert L.tetra_rx_unpack_bits(None, 1, 8, 60, None, 60) == -1


def test_rx_out_host_side_is_clean_under_asan_and_ubsan():
    """The reader, the unpacker and the layout arithmetic (csrc/rx_out_core.hpp) in a host-only build: deliveries truncated at every
    length and with every header word corrupted, read from exact-size heap blocks."""
    exe = os.path.join(SAN, "san_rx_out")
    srcs = [os.path.join(SAN, "san_rx_out.cpp")]
    deps = srcs + [os.path.join(PK, "csrc", "rx_out_core.hpp"), os.path.join(ROOT, "include", "tetra_rx_out.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + srcs + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "san_rx_out: ok" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- GPU

def _fetched(rx, which=0, kinds=range(6)):
    return {k: rx.fetch(k, which) for k in kinds}


def _assert_equal(got, want, packed, crc_good, ctx):
    assert sorted(got) == sorted(want), ctx
    for k, (wb, wt) in want.items():
        b, t = got[k]
        if crc_good:
            keep = wb["crc_ok"] != 0
            wb, wt = wb[keep], wt[keep]
        if packed:
            assert t.shape == (len(wb), PACKED_BYTES[k]), (ctx, k)
            t = np.unpackbits(t, axis=1)[:, :TYPE1[k]]
        assert b.tobytes() == wb.tobytes(), (ctx, k, len(b), len(wb))
        assert np.array_equal(t, wt), (ctx, k)


@pytest.mark.gpu
def test_gpu_rx_out_equals_fetch(pkg, synth):
    """which = 0 and 1, every kind, byte per bit and packed, all rows and CRC-good only, into mapped host memory and into device
    memory, and a kinds subset: row for row tetra_rx_fetch's rows."""
    import torch
    R = pkg.rx_binding
    Cn, nslots = 8, 72
    N = nslots * 510 // 2
    cells, tx, iq = _noisy_batch(synth, Cn, nslots, 2 * N, 9100)
    rx = pkg.RxChain(Cn, N)
    rx.process(iq[:, :N])
    rx.process(iq[:, N:])
    rx.wait()
    want = {w: _fetched(rx, w) for w in (0, 1)}
    assert sum(len(b) for b, _ in want[0].values()) > 500
    assert sum(int((b["crc_ok"] == 0).sum()) for b, _ in want[0].values()) > 0          # bad CRCs exist
    assert any(len(b) > 128 and len(b) % 128 for b, _ in want[0].values())              # a kind of several tiles, the last one partial
    for which in (0, 1):
        for packed in (False, True):
            for crc in (False, True):
                d = rx.deliver(which, packed=packed, crc_good_only=crc)
                got = d.wait()
                assert d.header.call == 1 - which and d.ready()
                _assert_equal(got, want[which], packed, crc, (which, packed, crc))
                for e in d.header.kinds[:d.header.n_kinds]:
                    assert e.n_rows_decoded == len(want[which][e.kind][0])
    # device destination
    dev = torch.device("cuda", 0)
    dbuf = torch.zeros(rx.out_bound(), dtype=torch.uint8, device=dev)
    got = rx.deliver(1, packed=True, crc_good_only=True, buf=dbuf).wait()
    _assert_equal(got, want[1], True, True, "device")
    # a kinds subset
    sub = (1 << R.KIND_SB2) | (1 << R.KIND_SCH_F)
    got = rx.deliver(0, kinds=sub).wait()
    _assert_equal(got, {k: want[0][k] for k in (R.KIND_SB2, R.KIND_SCH_F)}, False, False, "subset")
    rx.close()


@pytest.mark.gpu
def test_gpu_rx_out_streaming_deliveries_equal_one_call(pkg, synth):
    """The stream cut raggedly as in test_gpu_rx_streaming_calls_overlap_and_equal_one_call; call k's delivery is enqueued, then calls
    k + 1 and k + 2 before it is waited for (the tail of k + 2 must wait for it on the device).  The deliveries together equal one
    call over the whole stream, in two-stream and one-stream modes."""
    import torch
    R = pkg.rx_binding
    Cn, nslots = 4, 90
    N = nslots * 510 - 100
    cells, tx, iq = _downlink_batch(synth, Cn, nslots, N, 5000)
    one = pkg.RxChain(Cn, N)
    one.process(iq)
    one.wait()
    want = _fetched(one)
    one.close()
    dev = torch.device("cuda", 0)
    d_iq = torch.from_numpy(iq).to(dev)
    cuts = [0, 9000, 9001, 20000, 20180, 33000, N]
    for flags in (0, R.FLAG_ONE_STREAM):
        rx = pkg.RxChain(Cn, 16000, flags=flags)
        bufs = [R.HostBuffer(rx.out_bound(packed=True)) for _ in range(3)]
        s = torch.cuda.Stream(dev)
        pending, got = [], {k: [] for k in range(R.N_KINDS)}

        def drain(upto):
            while pending and pending[0][0] <= upto:
                _, d = pending.pop(0)
                for k, (b, t) in d.wait().items():
                    got[k] += _rows(b, np.unpackbits(t, axis=1)[:, :TYPE1[k]])

        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            enqueue(torch, rx, d_iq, a, b, s)
            pending.append((i + 2, rx.deliver(0, packed=True, buf=bufs[i % 3])))
            drain(i)                      # call k's delivery is read once calls k + 1 and k + 2 are enqueued
        drain(len(cuts))
        rx.wait()
        for k in range(R.N_KINDS):
            assert sorted(got[k]) == sorted(_rows(*want[k])), (flags, k, len(got[k]), len(want[k][0]))
        rx.close()
        for bf in bufs:
            bf.close()


@pytest.mark.gpu
def test_gpu_rx_out_statuses(pkg, synth):
    """Capacity one byte short: header status TETRA_ERR_SIZE with the exact size, nothing written past the header, the rows still
    fetchable.  Pageable memory: TETRA_ERR_ARG.  A kind the configuration does not decode: TETRA_ERR_UNSUPPORTED.  query 1 -> 0."""
    R = pkg.rx_binding
    L = pkg.load_library()
    Cn, nslots = 3, 40
    N = nslots * 510
    cells, tx, iq = _downlink_batch(synth, Cn, nslots, N, 6000)
    rx = pkg.RxChain(Cn, N, kinds=(1 << R.KIND_SCH_F) | (1 << R.KIND_BBK))
    with pytest.raises(pkg.TetraDemodError) as e:
        rx.deliver(0)
    assert e.value.status == -1                                    # no call yet
    rx.process(iq)
    d = rx.deliver(0)
    d.wait()
    hd = d.header
    assert hd.status == 0 and hd.n_kinds == 3                       # SB1 + BBK + SCH/F
    buf = R.HostBuffer(hd.bytes + 4096)
    buf.array[:] = 0xA5
    call = C.c_int64(-1)
    assert L.tetra_rx_out_enqueue(rx._h, 0, 0, 0, C.c_void_p(buf.ptr), hd.bytes - 1, C.byref(call)) == 0
    assert L.tetra_rx_out_wait(rx._h, call) == 0
    h2 = R.OutHeader.from_buffer_copy(buf.array[:C.sizeof(R.OutHeader)].tobytes())
    assert h2.magic == R.OUT_MAGIC and h2.status == -6 and h2.bytes == hd.bytes
    assert (buf.array[C.sizeof(R.OutHeader):] == 0xA5).all()      # nothing past the header
    b, t = rx.fetch(R.KIND_SCH_F)
    assert len(b) > 10
    assert L.tetra_rx_out_enqueue(rx._h, 0, 0, 0, C.c_void_p(buf.ptr), 223, C.byref(call)) == -6
    # pageable memory, an unconfigured kind, bad arguments
    pageable = np.zeros(hd.bytes, np.uint8)
    with pytest.raises(pkg.TetraDemodError) as e:
        rx.deliver(0, buf=pageable)
    assert e.value.status == -1
    with pytest.raises(pkg.TetraDemodError) as e:
        rx.deliver(0, kinds=1 << R.KIND_SB2)
    assert e.value.status == -2
    assert L.tetra_rx_out_enqueue(rx._h, 0, 1 << 6, 0, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == -1
    assert L.tetra_rx_out_enqueue(rx._h, 0, 0, 4, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == -1
    assert L.tetra_rx_out_query(rx._h, 5) == -1
    # query moves from pending to done: a delivery enqueued right behind a fresh call waits for that call's tail on the device
    rx.process(iq)
    d = rx.deliver(0, buf=buf)
    seen = [L.tetra_rx_out_query(rx._h, d.call)]
    while seen[-1] == 1 and len(seen) < 10 ** 7:
        seen.append(L.tetra_rx_out_query(rx._h, d.call))
    assert seen[0] == 1 and seen[-1] == 0 and set(seen) == {0, 1}
    assert d.ready() and len(d.wait()[R.KIND_SCH_F][0]) == len(rx.fetch(R.KIND_SCH_F)[0])
    rx.close()
    buf.close()


@pytest.mark.gpu
def test_gpu_rx_out_multibank_fetch_all_equals_fetch(pkg, synth, tmp_path):
    """TetraRxMultiBank::fetchAll (every shard's delivery enqueued first, then collected) with 3 shards on one GPU equals fetch of
    each kind, byte per bit and packed + CRC-good only; a plain C++ driver (tests/host/test_rx_out_multibank.cpp)."""
    pkg.build.build()
    exe = os.path.join(ROOT, "tests", "host", "test_rx_out_multibank")
    src = os.path.join(ROOT, "tests", "host", "test_rx_out_multibank.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PK, "host"), src,
                    "-L", PK, "-ltetra_demod_hip", "-Wl,-rpath," + PK, "-o", exe], check=True)
    Cn, calls, nslots = 7, 3, 48
    N = nslots * 510 // calls
    cells, tx, iq = _noisy_batch(synth, Cn, nslots, N * calls, 8900)
    f = tmp_path / "iq.bin"
    with open(f, "wb") as fh:
        for k in range(calls):
            fh.write(np.ascontiguousarray(iq[:, k * N:(k + 1) * N]).astype(np.complex64).tobytes())
    for flags in (0, 3):
        r = subprocess.run([exe, str(Cn), str(N), str(calls), str(f), "3", str(flags)], capture_output=True, text=True, timeout=180)
        assert r.returncode == 0 and "test_rx_out_multibank: ok" in r.stdout, (flags, r.stdout[-500:], r.stderr[-2000:])
        assert int(r.stdout.split()[2]) > 300
