"""The opt-in row extras and per-channel state through the one-step hand-off (include/ext/tetra_rx_out_ext.h): the documented layout
against the host readers, the host side under sanitizers, the extras writer's lane code against numpy's column[keep], the ABI, and on the
GPU the extended deliveries against the blocking fetches and getters they replace."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests.rx_out_reference import CHAN_BYTES, a16 as _a16, build_ext_delivery as _build_ext_delivery, keep_patterns as _keep_patterns
from tests.chain_gpu import enqueue
from tests.chain_host import downlink_batch as _downlink_batch, noisy_batch as _noisy_batch
from tests.test_rx_out import _build_delivery

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PK = os.path.join(ROOT, "sdrpp-tetra-demodulator_amd")
SAN = os.path.join(ROOT, "tests", "san")
HDR = os.path.join(ROOT, "include", "ext", "tetra_rx_out_ext.h")
ROW_BYTES = [4, 4, 1]
ARG, UNSUPPORTED, SIZE = -1, -2, -6


# ---------------------------------------------------------------------------------------------------------------- ABI

def test_rx_out_ext_header_is_exported_and_bound(pkg):
    """The functions include/ext/tetra_rx_out_ext.h declares are the binding's RX_OUT_EXT_EXPORTS, each exported by the library with as
    many parameters as declared; the header compiles as C; tetra_rx_out.h's own list is untouched by them."""
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    decls = {m.group(1): " ".join(m.group(2).split()).split(",") for m in re.finditer(r"\bint\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}
    R = pkg.rx_binding
    assert len(decls) == 5 and set(decls) == set(R.RX_OUT_EXT_EXPORTS) == set(R.OUT_EXT_ABI)
    assert not set(decls) & (set(R.RX_OUT_EXPORTS) | set(R.RX_EXPORTS))
    L = pkg.load_library()
    R._lib()
    for name, params in decls.items():
        fn = getattr(L, name)
        assert len(R.OUT_EXT_ABI[name][1]) == len(params) == len(fn.argtypes), name
        for decl, ct in zip(params, R.OUT_EXT_ABI[name][1]):
            if decl.strip().startswith(("uint64_t ", "int64_t ")):
                assert C.sizeof(ct) == 8, (name, decl)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", HDR], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c++", HDR], check=True)


def test_rx_out_ext_struct_layouts_match_header(pkg):
    R = pkg.rx_binding
    K, H = "tetra_rx_out_ext_kind_t", "tetra_rx_out_ext_header_t"
    exprs = (["sizeof(%s)" % K, "sizeof(%s)" % H] + ["offsetof(%s, %s)" % (K, f) for f, _ in R.OutExtKind._fields_] +
             ["offsetof(%s, %s)" % (H, f) for f, _ in R.OutExtHeader._fields_] +
             ["sizeof(tetra_lmac_cell_state_t)", "sizeof(tetra_bsync_state_t)", "sizeof(tetra_rx_link_t)",
              "offsetof(tetra_rx_link_t, bit_errors)", "offsetof(tetra_rx_link_t, blocks)", "offsetof(tetra_rx_link_t, blocks_crc_bad)",
              "offsetof(tetra_bsync_state_t, next_frame_start_bitnum)", "offsetof(tetra_lmac_cell_state_t, phy_mn)"] +
             ["TETRA_RX_OUT_EXT_" + n for n in ("ROW_BITERR", "ROW_LIST_RANK", "ROW_AACH_DIST", "CHAN_CELL", "CHAN_SYNC_STATE", "CHAN_SYNC_MISSES",
                                                "CHAN_LINK", "ROW_ALL", "CHAN_ALL", "MAGIC")])
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ext/tetra_rx_out_ext.h"\nint main(){' +
            "".join('printf("%%llu\\n", (unsigned long long)(%s));' % e for e in exprs) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as td:
        cfile, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(cfile, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = ([C.sizeof(R.OutExtKind), C.sizeof(R.OutExtHeader)] + [getattr(R.OutExtKind, f).offset for f, _ in R.OutExtKind._fields_] +
            [getattr(R.OutExtHeader, f).offset for f, _ in R.OutExtHeader._fields_] +
            [R.CELL_DTYPE.itemsize, R.SYNC_STATE_DTYPE.itemsize, R.LINK_DTYPE.itemsize, R.LINK_DTYPE.fields["bit_errors"][1],
             R.LINK_DTYPE.fields["blocks"][1], R.LINK_DTYPE.fields["blocks_crc_bad"][1], R.SYNC_STATE_DTYPE.fields["next_frame_start_bitnum"][1],
             R.CELL_DTYPE.fields["phy_mn"][1]] +
            [R.EXT_ROW_BITERR, R.EXT_ROW_LIST_RANK, R.EXT_ROW_AACH_DIST, R.EXT_CHAN_CELL, R.EXT_CHAN_SYNC_STATE, R.EXT_CHAN_SYNC_MISSES, R.EXT_CHAN_LINK,
             R.EXT_ROW_ALL, R.EXT_CHAN_ALL, R.OUT_EXT_MAGIC])
    assert v == want
    assert C.sizeof(R.OutExtHeader) == 256 and [R.CELL_DTYPE.itemsize, R.SYNC_STATE_DTYPE.itemsize, 4, R.LINK_DTYPE.itemsize] == CHAN_BYTES
    assert C.sizeof(R.CellState) == 40 and C.sizeof(R.Link) == 24


# ---------------------------------------------------------------------------------------------------------------- layout and readers

def _view_ext_rc(L, buf, nbytes, kind):
    return L.tetra_rx_out_view_ext(buf.ctypes.data_as(C.c_void_p), nbytes, kind, None, None, None, None)


def _view_chan_rc(L, buf, nbytes):
    return L.tetra_rx_out_view_channels(buf.ctypes.data_as(C.c_void_p), nbytes, None, None, None, None, None)


def test_rx_out_ext_views_read_the_documented_layout(pkg):
    R = pkg.rx_binding
    L = R._lib()
    rng = np.random.default_rng(15)
    rows = {0: 3, 1: 17, 3: 0, 5: 9, 2: 129}
    Cn = 5
    for flags in (0, R.OUT_PACKED, R.OUT_CRC_GOOD, R.OUT_PACKED | R.OUT_CRC_GOOD):
        for extras in (247, R.EXT_ROW_BITERR, R.EXT_ROW_AACH_DIST | R.EXT_CHAN_SYNC_MISSES, R.EXT_ROW_LIST_RANK | R.EXT_CHAN_CELL | R.EXT_CHAN_LINK,
                       R.EXT_CHAN_SYNC_STATE):
            buf, want, cols, tabs, bounds = _build_ext_delivery(R, rows, flags, extras, Cn, rng)
            ctx = (flags, extras)
            ex, gcols, gch = R.view_delivery_ext(buf)
            assert ex.bytes == buf.nbytes and ex.extras == extras and ex.call == 41 and ex.n_channels == Cn, ctx
            for k in rows:
                for c, name in enumerate(("biterr", "rank", "aach_dist")):
                    g, w = gcols[k][name], cols[k][c]
                    assert (g is None) == (w is None), (ctx, k, name)
                    assert g is None or (g.dtype == w.dtype and g.tobytes() == w.tobytes() and len(g) == rows[k]), (ctx, k, name)
            for t, name in enumerate(("cell", "sync_state", "sync_misses", "link")):
                assert (gch[name] is None) == (tabs[t] is None), (ctx, name)
                assert tabs[t] is None or (gch[name].tobytes() == tabs[t] and len(gch[name]) == Cn), (ctx, name)
            # the classic reader still reads the same buffer
            hd, got = R.view_delivery(buf)
            assert sorted(got) == sorted(rows) and hd.bytes < buf.nbytes
            for k in rows:
                assert got[k][0].tobytes() == want[k][0].tobytes() and np.array_equal(got[k][1], want[k][1]), (ctx, k)
            # truncated at every section boundary and one byte short of the total: refused; a classic-only buffer has no extension
            for cut in bounds[:-1] + [buf.nbytes - 1]:
                assert _view_ext_rc(L, buf, cut, 5) in (ARG, UNSUPPORTED) and _view_chan_rc(L, buf, cut) in (ARG, UNSUPPORTED), (ctx, cut)
            assert _view_ext_rc(L, buf, int(hd.bytes), 5) == UNSUPPORTED and _view_chan_rc(L, buf, int(hd.bytes)) == UNSUPPORTED
            assert _view_ext_rc(L, buf, buf.nbytes - 1, 5) == ARG and _view_chan_rc(L, buf, buf.nbytes - 1) == ARG
            assert _view_ext_rc(L, buf, buf.nbytes, 4) == UNSUPPORTED and _view_ext_rc(L, buf, buf.nbytes, 6) == ARG      # a kind not held / no kind
            at = _a16(int(hd.bytes))

            def corrupt(kind_entry, field, value):
                bad = buf.copy()
                e2 = R.OutExtHeader.from_buffer(bad, at)
                setattr(e2 if kind_entry is None else e2.kinds[kind_entry], field, value)
                del e2
                return bad

            for field, value in (("magic", R.OUT_MAGIC), ("bytes", buf.nbytes + 1), ("call", 40), ("extras", 256), ("n_kinds", 3)):
                bad = corrupt(None, field, value)
                assert _view_ext_rc(L, bad, bad.nbytes, 5) == ARG and _view_chan_rc(L, bad, bad.nbytes) == ARG, (ctx, field)
            bad = corrupt(4, "n_rows", 8)              # kind 5's entry disagrees with the classic one
            assert _view_ext_rc(L, bad, bad.nbytes, 5) == ARG, ctx
            if extras & R.EXT_ROW_BITERR:
                for value in (buf.nbytes + 16, buf.nbytes - 16, ex.kinds[4].biterr_offset + 4, 16):      # outside, too close to the end, misaligned, in the classic part
                    bad = corrupt(4, "biterr_offset", value)
                    assert _view_ext_rc(L, bad, bad.nbytes, 5) == ARG, (ctx, value)
            if extras & R.EXT_CHAN_CELL:
                for value in (buf.nbytes + 16, _a16(buf.nbytes) - 16, ex.cell_offset + 8, 224):
                    bad = corrupt(None, "cell_offset", value)
                    assert _view_chan_rc(L, bad, bad.nbytes) == ARG, (ctx, value)
    # the classic delivery of test_rx_out: no extension block
    buf, _ = _build_delivery(R, {0: 3, 1: 17, 3: 0, 5: 9}, 0, rng)
    assert _view_ext_rc(L, buf, buf.nbytes, 5) == UNSUPPORTED and _view_chan_rc(L, buf, buf.nbytes) == UNSUPPORTED


def test_rx_out_ext_host_side_is_clean_under_asan_and_ubsan():
    """csrc/rx_out_core.hpp's extension code as a stand-alone host program (tests/san/san_rx_out_ext.cpp): extended deliveries written by
    the lane code, truncated at every length and with every word of both headers flipped, in exact-size heap blocks."""
    exe = os.path.join(SAN, "san_rx_out_ext")
    srcs = [os.path.join(SAN, "san_rx_out_ext.cpp")]
    deps = srcs + [os.path.join(PK, "csrc", "rx_out_core.hpp"), os.path.join(ROOT, "include", "tetra_rx_out.h"), HDR]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all"] + srcs + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "san_rx_out_ext: ok" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])


# ---------------------------------------------------------------------------------------------------------------- the writer's lane code

def test_rx_out_ext_lane_code_writes_column_of_keep():
    """The columns the tiles write (host build of the lane code, tests/emul/rx_out_ext_emul.cpp) are numpy's column[keep], at every
    tile edge, for every keep pattern, and with the run starting at every residue of 16 bytes; nothing else of the buffer changes."""
    from tests.emul import rx_out_ext_emul_bind as E
    L = E.lib()
    rng = np.random.default_rng(21)
    for n in (0, 1, 127, 128, 129, 257, 640):
        col4 = rng.integers(0, 2 ** 32, max(n, 1), dtype=np.uint64).astype(np.uint32)
        t2 = rng.integers(0, 256, (max(n, 1), 32)).astype(np.uint8)
        for name, ok in _keep_patterns(n).items():
            for crc in (0, 1):
                keep = ok != 0 if crc else np.ones(n, bool)
                for elem, src, want in ((4, col4, col4[:n][keep]), (1, t2, t2[:n, 30][keep])):
                    for first in range(0, 16, elem) if elem == 1 else range(4):      # first output row -> the run's first byte at every residue
                        col_off = 64
                        dst = np.full(col_off + elem * (first + n) + 64, 0xA5, np.uint8)
                        assert dst.ctypes.data % 16 == 0
                        L.rx_out_ext_emul_column(src.ctypes.data, elem, 32, 30, ok.ctypes.data, n, crc, col_off, first, dst.ctypes.data)
                        a = col_off + elem * first
                        got = dst[a: a + elem * len(want)]
                        assert got.tobytes() == want.tobytes(), (n, name, crc, elem, first)
                        dst[a: a + elem * len(want)] = 0xA5
                        assert (dst == 0xA5).all(), (n, name, crc, elem, first)
    # per-channel tables: whole 16-byte units and the 4-byte words at the end, any number of workgroups
    for nbytes in (0, 4, 12, 16, 20, 40 * 3, 24 * 4096 + 8):
        src = np.zeros(nbytes + 16, np.uint8)[:nbytes]
        src[:] = rng.integers(0, 256, nbytes)
        for groups in (1, 3):
            dst = np.full(nbytes + 32, 0xA5, np.uint8)
            L.rx_out_ext_emul_table(src.ctypes.data, nbytes, groups, dst.ctypes.data)
            assert dst[:nbytes].tobytes() == src.tobytes() and (dst[nbytes:] == 0xA5).all(), (nbytes, groups)


def test_rx_out_ext_layout_arithmetic_is_the_documented_one(pkg):
    """rx_out::layout_ext (what the layout workgroup runs) gives the offsets of the hand-built delivery, and the snapshot's tables are
    16-byte aligned."""
    from tests.emul import rx_out_ext_emul_bind as E
    R = pkg.rx_binding
    L = E.lib()
    rng = np.random.default_rng(3)
    rows = {0: 3, 1: 17, 2: 129, 3: 0, 5: 9}
    kinds = np.array(sorted(rows), np.int32)
    n_rows = np.array([rows[k] for k in kinds], np.int32)
    for flags in range(4):
        for extras in (247, 1, 4 | 64, 2 | 16 | 128, 32, 0):
            buf, _, _, _, _ = _build_ext_delivery(R, rows, flags, extras, 7, rng)
            hd, ex = R.OutHeader(), R.OutExtHeader()
            total = L.rx_out_ext_emul_layout(kinds.ctypes.data, n_rows.ctypes.data, len(kinds), flags, extras, 7, C.byref(hd), C.byref(ex))
            assert total == buf.nbytes == ex.bytes
            ex.magic, ex.call = R.OUT_EXT_MAGIC, 41
            at = _a16(int(hd.bytes))
            assert bytes(ex) == buf[at: at + 256].tobytes(), (flags, extras)
    for Cn in (1, 3, 4096):
        offs = [L.rx_out_ext_emul_snap_offset(t, Cn) for t in range(5)]
        assert all(o % 16 == 0 for o in offs) and all(b - a >= CHAN_BYTES[t] * Cn for t, (a, b) in enumerate(zip(offs, offs[1:])))


# ---------------------------------------------------------------------------------------------------------------- GPU

SEED = 9100          # tests/test_rx_out.py's noisy batch: 8 channels, 72 slots, the last two at 6 dB
ALL_ROW, ALL_CHAN = 7, 240


def _ext_flags(R):
    return R.FLAG_BITERR | R.FLAG_LIST | R.FLAG_AACH_RM3014 | R.FLAG_SYNC_TOLERANT


def test_the_chosen_seed_meets_the_preconditions_on_the_cpu(synth, oracle):
    """On the CPU, from the oracle demodulator's bits of the two noisy channels and tests/list_pipeline.py (reference synchroniser, the
    numpy decoder with four candidates): CRC-bad coded rows, rows with errors > 0 and rescued rows exist in the input that
    test_gpu_rx_out_ext_equals_the_blocking_fetches uses.  (The AACH distance is not part of that pipeline: see there.)"""
    from tests import list_pipeline as LP
    Cn, nslots = 8, 72
    N = nslots * 510 // 2
    _, _, iq = _noisy_batch(synth, Cn, nslots, 2 * N, SEED)
    bits, nb = oracle.process_batch(np.array(iq[Cn - 2:]))[:2]
    rows = {}
    for c in range(2):
        rows.update(LP.channel_rows(oracle, bits[c][:nb[c]], c, 4))
    assert sum(1 for v in rows.values() if v[0] == 0) > 0
    assert sum(1 for v in rows.values() if v[5][0] > 0) > 0
    assert sum(1 for v in rows.values() if v[4] > 0) > 0


def _cells_array(R, cells):
    return np.frombuffer(b"".join(bytes(c) for c in cells), R.CELL_DTYPE)


def _blocking_tables(R, rx):
    """the four per-channel tables through the blocking getters, as the delivery's dtypes"""
    links = rx.links()
    link = np.zeros(len(links), R.LINK_DTYPE)
    for i, l in enumerate(links):
        link[i] = (l["bits"], l["bit_errors"], l["blocks"], l["blocks_crc_bad"])
    sync = np.array(rx.sync_states(), dtype=np.int64)
    st = np.zeros(len(sync), R.SYNC_STATE_DTYPE)
    for j, f in enumerate(R.SYNC_STATE_DTYPE.names):
        st[f] = sync[:, j]
    return dict(cell=_cells_array(R, rx.cells()), sync_state=st, sync_misses=rx.sync_misses().astype("<i4"), link=link)


def _assert_tables(got, want, ctx):
    for name, w in want.items():
        assert got[name] is not None and got[name].tobytes() == w.tobytes(), (ctx, name)


@pytest.mark.gpu
def test_gpu_rx_out_ext_equals_the_blocking_fetches(pkg, synth):
    """which = 0 and 1, the four flag combinations, every extra on: the buffer's first header.bytes bytes are the classic delivery of the
    same call, every column is its blocking fetch (filtered by crc_ok under CRC_GOOD), and the channel tables of which = 0 are the
    blocking getters' read right after; once into device memory, once with kinds that have none of a given extra.
    The seed's preconditions -- a CRC-bad coded row, a row with errors > 0, a rank other than 0 -- are checked on the CPU by
    test_the_chosen_seed_meets_the_preconditions_on_the_cpu with the reference pipeline (which runs the reference's synchroniser, while
    this handle runs the tolerant lock: the assertions below are on the chain's own rows).  An AACH distance above 0 cannot be checked
    there: the pipeline has no AACH decoder; the assertion stands here."""
    import torch
    R = pkg.rx_binding
    Cn, nslots = 8, 72
    N = nslots * 510 // 2
    _, _, iq = _noisy_batch(synth, Cn, nslots, 2 * N, SEED)
    rx = pkg.RxChain(Cn, N, flags=_ext_flags(R))
    rx.set_snapshot(ALL_CHAN)
    rx.process(iq[:, :N])
    rx.process(iq[:, N:])
    rx.wait()
    coded = [k for k in range(6) if k != R.KIND_BBK]
    want, be, rank, dist = {}, {}, {}, {}
    for w in (0, 1):
        want[w] = {k: rx.fetch(k, w) for k in range(6)}
        be[w] = {k: rx._count_then_fetch(rx._lib.tetra_rx_fetch_biterr, np.uint32, w, k) for k in coded}
        rank[w] = {k: rx.fetch_list_rank(k, w) for k in coded}
        dist[w] = rx.fetch_aach_dist(w)
    tables = _blocking_tables(R, rx)
    # preconditions, so that nothing below passes vacuously
    assert sum(int((want[0][k][0]["crc_ok"] == 0).sum()) for k in coded) > 0
    assert sum(int(((be[0][k] & 0xffff) > 0).sum()) for k in coded) > 0
    assert sum(int((rank[0][k] != 0).sum()) for k in coded) > 0
    assert int(((dist[0] > 0) & (dist[0] != R.AACH_UNDECODABLE)).sum()) > 0
    assert any(len(b) > 128 and len(b) % 128 for b, _ in want[0].values())
    assert sum(int(m) for m in tables["sync_misses"]) >= 0 and tables["link"]["blocks"].sum() > 0 and tables["cell"]["mcc"].any()

    def check(d, got, which, crc, kinds, ctx):
        assert d.ext_header.call == d.header.call == 1 - which and d.ext_header.n_channels == Cn, ctx
        for k in kinds:
            keep = want[which][k][0]["crc_ok"] != 0 if crc else np.ones(len(want[which][k][0]), bool)
            assert got[k][0].tobytes() == want[which][k][0][keep].tobytes(), (ctx, k)
            c = got.columns[k]
            if k == R.KIND_BBK:
                assert c["biterr"] is None and c["rank"] is None and np.array_equal(c["aach_dist"], dist[which][keep]), (ctx, k)
            else:
                assert c["aach_dist"] is None and np.array_equal(c["biterr"], be[which][k][keep]) and np.array_equal(c["rank"], rank[which][k][keep]), (ctx, k)

    for which in (0, 1):
        for packed in (False, True):
            for crc in (False, True):
                ctx = (which, packed, crc)
                ext = R.HostBuffer(rx.out_bound(packed=packed, crc_good_only=crc, extras=ALL_ROW | ALL_CHAN))
                ext.array[:] = 0xA5
                d = rx.deliver(which, packed=packed, crc_good_only=crc, buf=ext, extras=ALL_ROW | ALL_CHAN)
                got = d.wait()
                assert d.ext_header.extras == ALL_ROW | ALL_CHAN and d.ext_header.bytes <= ext.nbytes, ctx
                cl = R.HostBuffer(rx.out_bound(packed=packed, crc_good_only=crc))
                cl.array[:] = 0xA5                     # (the padding between sections is written by neither)
                classic = rx.deliver(which, packed=packed, crc_good_only=crc, buf=cl)
                classic.wait()
                nb = int(classic.header.bytes)
                assert d.header.bytes == nb and ext.array[:nb].tobytes() == cl.array[:nb].tobytes(), ctx
                cl.close()
                assert (ext.array[int(d.ext_header.bytes):] == 0xA5).all(), ctx            # nothing behind the total
                check(d, got, which, crc, range(6), ctx)
                if which == 0:
                    _assert_tables(got.channels, tables, ctx)
                ext.close()
    # device destination
    dev = torch.device("cuda", 0)
    dbuf = torch.zeros(rx.out_bound(extras=ALL_ROW | ALL_CHAN), dtype=torch.uint8, device=dev)
    d = rx.deliver(0, packed=True, crc_good_only=True, buf=dbuf, extras=ALL_ROW | ALL_CHAN)
    got = d.wait()
    check(d, got, 0, True, range(6), "device")
    _assert_tables(got.channels, tables, "device")
    # kinds without any column of a given extra: no error, the bit is not delivered
    d = rx.deliver(0, kinds=1 << R.KIND_BBK, extras=R.EXT_ROW_BITERR | R.EXT_ROW_LIST_RANK | R.EXT_CHAN_LINK)
    got = d.wait()
    assert d.ext_header.extras == R.EXT_CHAN_LINK and got.columns[R.KIND_BBK] == dict(biterr=None, rank=None, aach_dist=None)
    assert got.channels["link"].tobytes() == tables["link"].tobytes() and got.channels["cell"] is None
    d = rx.deliver(0, kinds=(1 << R.KIND_SB2) | (1 << R.KIND_SCH_F), crc_good_only=True, extras=ALL_ROW)
    got = d.wait()
    assert d.ext_header.extras == R.EXT_ROW_BITERR | R.EXT_ROW_LIST_RANK
    check(d, got, 0, True, (R.KIND_SB2, R.KIND_SCH_F), "subset")
    rx.close()


@pytest.mark.gpu
def test_gpu_rx_out_ext_snapshot_is_the_delivered_calls_state(pkg, synth):
    """The ragged cuts of test_gpu_rx_out_streaming_deliveries_equal_one_call: call k's extended delivery is enqueued, calls k + 1 and
    k + 2 are processed before it is waited for, and its channel tables equal those of a second handle fed the same stream, stopped
    after call k and read with the blocking getters -- the snapshot, not the live arrays, which have moved on by then."""
    import torch
    R = pkg.rx_binding
    Cn, nslots = 4, 90
    N = nslots * 510 - 100
    _, _, iq = _downlink_batch(synth, Cn, nslots, N, 5000)
    dev = torch.device("cuda", 0)
    d_iq = torch.from_numpy(iq).to(dev)
    cuts = [0, 9000, 9001, 20000, 20180, 33000, N]
    for flags in (0, R.FLAG_ONE_STREAM):
        # the second handle first: the same stream, stopped after every call and read with the blocking getters
        ref = pkg.RxChain(Cn, 16000, flags=flags | _ext_flags(R))
        want = []
        for a, b in zip(cuts, cuts[1:]):
            ref.process_device(d_iq[:, a:b].contiguous(), b - a, None)
            want.append(_blocking_tables(R, ref))
        rx = pkg.RxChain(Cn, 16000, flags=flags | _ext_flags(R))
        rx.set_snapshot(ALL_CHAN)
        bufs = [R.HostBuffer(rx.out_bound(packed=True, extras=ALL_CHAN)) for _ in range(4)]
        s = torch.cuda.Stream(dev)
        pending, got = [], []
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            enqueue(torch, rx, d_iq, a, b, s)
            pending.append((i + 2, rx.deliver(0, packed=True, buf=bufs[i % 3], extras=ALL_CHAN)))
            while pending and pending[0][0] <= i:           # call k's delivery is read once calls k + 1 and k + 2 are enqueued
                got.append({k: v.copy() for k, v in pending.pop(0)[1].wait().channels.items()})
            if i >= 1:      # and the previous call's, enqueued behind this call's tail: the live arrays are a call further by then
                prev = rx.deliver(1, kinds=1 << R.KIND_SB1, buf=bufs[3], extras=ALL_CHAN).wait()
                _assert_tables(prev.channels, want[i - 1], (flags, i, "which = 1"))
        for _, d in pending:
            got.append({k: v.copy() for k, v in d.wait().channels.items()})
        rx.wait()
        assert len(got) == len(want) == len(cuts) - 1
        for k, (g, w) in enumerate(zip(got, want)):
            _assert_tables(g, w, (flags, k))
        # the state moves from call to call, so a read of the live arrays would have been noticed
        for name in ("cell", "sync_state", "link"):
            assert sum(want[k][name].tobytes() != want[k + 1][name].tobytes() for k in range(len(want) - 1)) >= 3, (flags, name)
        rx.close()
        ref.close()
        for bf in bufs:
            bf.close()


@pytest.mark.gpu
def test_gpu_rx_out_ext_statuses(pkg, synth):
    """One byte short of the total: the classic header alone, TETRA_ERR_SIZE with the total, nothing past it.  An extra without its
    handle flag: TETRA_ERR_UNSUPPORTED.  A channel extra without an armed snapshot, or armed after the call: TETRA_ERR_ARG.  An unknown
    bit: TETRA_ERR_ARG.  extras = 0: tetra_rx_out_enqueue's bytes."""
    R = pkg.rx_binding
    L = R._lib()
    Cn, nslots = 3, 40
    N = nslots * 510
    _, _, iq = _downlink_batch(synth, Cn, nslots, N, 6000)
    rx = pkg.RxChain(Cn, N, flags=_ext_flags(R))
    rx.set_snapshot(ALL_CHAN)
    rx.process(iq)
    every = ALL_ROW | ALL_CHAN
    d = rx.deliver(0, extras=every)
    d.wait()
    total, classic = int(d.ext_header.bytes), int(d.header.bytes)
    assert total > classic + 256 and rx.out_bound(extras=every) >= total
    buf = R.HostBuffer(rx.out_bound(extras=every) + 4096)      # (the worst case of this shape: also enough for the second handle below)
    call = C.c_int64(-1)
    for cap in (total - 1, classic, classic - 1):
        buf.array[:] = 0xA5
        assert L.tetra_rx_out_enqueue_ext(rx._h, 0, 0, 0, every, C.c_void_p(buf.ptr), cap, C.byref(call)) == 0
        assert L.tetra_rx_out_wait(rx._h, call) == 0
        h2 = R.OutHeader.from_buffer_copy(buf.array[:224].tobytes())
        assert h2.magic == R.OUT_MAGIC and h2.status == SIZE and h2.bytes == total, cap
        assert (buf.array[224:] == 0xA5).all(), cap
    buf.array[:] = 0xA5
    assert L.tetra_rx_out_enqueue_ext(rx._h, 0, 0, 0, every, C.c_void_p(buf.ptr), total, C.byref(call)) == 0       # exactly the total fits
    assert L.tetra_rx_out_wait(rx._h, call) == 0
    assert R.OutHeader.from_buffer_copy(buf.array[:224].tobytes()).status == 0 and (buf.array[total:] == 0xA5).all()
    R.view_delivery_ext(buf, total)
    # extras = 0: byte for byte tetra_rx_out_enqueue
    b0, b1 = R.HostBuffer(classic + 512), R.HostBuffer(classic + 512)
    for b, fn, extra in ((b0, L.tetra_rx_out_enqueue, ()), (b1, L.tetra_rx_out_enqueue_ext, (0,))):
        b.array[:] = 0xA5
        assert fn(rx._h, 0, 0, R.OUT_CRC_GOOD, *extra, C.c_void_p(b.ptr), b.nbytes, C.byref(call)) == 0
        assert L.tetra_rx_out_wait(rx._h, call) == 0
    assert b0.array.tobytes() == b1.array.tobytes() and (b1.array[classic:] == 0xA5).all()
    # unknown bits
    for bad in (8, 256, -1, 1 << 20):
        assert L.tetra_rx_out_enqueue_ext(rx._h, 0, 0, 0, bad, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == ARG, bad
    assert L.tetra_rx_out_set_snapshot(rx._h, R.EXT_ROW_BITERR) == ARG and L.tetra_rx_out_set_snapshot(rx._h, 256) == ARG
    nb = C.c_uint64(0)
    assert L.tetra_rx_out_bound_ext(rx._h, 0, 0, 8, C.byref(nb)) == ARG and L.tetra_rx_out_bound_ext(rx._h, 0, 4, 0, C.byref(nb)) == ARG
    rx.close()
    # a handle without the flags: every flagged extra is unsupported, as its blocking fetch answers; cell and state always can
    plain = pkg.RxChain(Cn, N)
    plain.process(iq)
    for extra in (R.EXT_ROW_BITERR, R.EXT_ROW_LIST_RANK, R.EXT_ROW_AACH_DIST, R.EXT_CHAN_SYNC_MISSES, R.EXT_CHAN_LINK):
        assert L.tetra_rx_out_enqueue_ext(plain._h, 0, 0, 0, extra, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == UNSUPPORTED, extra
        assert L.tetra_rx_out_bound_ext(plain._h, 0, 0, extra, C.byref(nb)) == UNSUPPORTED, extra
    assert L.tetra_rx_out_set_snapshot(plain._h, R.EXT_CHAN_LINK) == UNSUPPORTED and L.tetra_rx_out_set_snapshot(plain._h, R.EXT_CHAN_SYNC_MISSES) == UNSUPPORTED
    # no snapshot armed: TETRA_ERR_ARG; armed after the call: still TETRA_ERR_ARG for that call, fine for the next; reset invalidates, keeps the mask
    assert L.tetra_rx_out_enqueue_ext(plain._h, 0, 0, 0, R.EXT_CHAN_CELL, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == ARG
    plain.set_snapshot(R.EXT_CHAN_CELL)
    assert L.tetra_rx_out_enqueue_ext(plain._h, 0, 0, 0, R.EXT_CHAN_CELL, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == ARG
    plain.process(iq)
    assert L.tetra_rx_out_enqueue_ext(plain._h, 1, 0, 0, R.EXT_CHAN_CELL, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == ARG
    assert L.tetra_rx_out_enqueue_ext(plain._h, 0, 0, 0, R.EXT_CHAN_SYNC_STATE, C.c_void_p(buf.ptr), buf.nbytes, C.byref(call)) == ARG
    got = plain.deliver(0, buf=buf, extras=R.EXT_CHAN_CELL).wait()
    assert got.channels["cell"].tobytes() == _cells_array(R, plain.cells()).tobytes()
    plain.reset()
    plain.process(iq)
    got = plain.deliver(0, buf=buf, extras=R.EXT_CHAN_CELL).wait()
    assert got.channels["cell"].tobytes() == _cells_array(R, plain.cells()).tobytes()
    plain.set_sync_tolerance((3, 5, 16))          # a set tolerance makes the miss counters deliverable
    plain.set_snapshot(R.EXT_CHAN_SYNC_MISSES)
    plain.process(iq)
    got = plain.deliver(0, buf=buf, extras=R.EXT_CHAN_SYNC_MISSES).wait()
    assert np.array_equal(got.channels["sync_misses"], plain.sync_misses())
    plain.close()
    for b in (buf, b0, b1):
        b.close()


@pytest.mark.gpu
def test_gpu_rx_out_ext_multibank_fetch_all_equals_the_blocking_fetches(pkg, synth, tmp_path):
    """TetraRxMultiBank::fetchAll with extras on 2 shards of the one GPU against the per-shard blocking fetches and getters, row for row
    and channel for channel; a plain C++ driver (tests/host/test_rx_out_ext_multibank.cpp)."""
    pkg.build.build()
    exe = os.path.join(ROOT, "tests", "host", "test_rx_out_ext_multibank")
    src = os.path.join(ROOT, "tests", "host", "test_rx_out_ext_multibank.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PK, "host"), src,
                    "-L", PK, "-ltetra_demod_hip", "-Wl,-rpath," + PK, "-o", exe], check=True)
    Cn, calls, nslots = 7, 3, 48
    N = nslots * 510 // calls
    _, _, iq = _noisy_batch(synth, Cn, nslots, N * calls, 8900)
    f = tmp_path / "iq.bin"
    with open(f, "wb") as fh:
        for k in range(calls):
            fh.write(np.ascontiguousarray(iq[:, k * N:(k + 1) * N]).astype(np.complex64).tobytes())
    for flags in (0, 3):
        r = subprocess.run([exe, str(Cn), str(N), str(calls), str(f), "2", str(flags)], capture_output=True, text=True, timeout=180)
        assert r.returncode == 0 and "test_rx_out_ext_multibank: ok" in r.stdout, (flags, r.stdout[-500:], r.stderr[-2000:])
        assert int(r.stdout.split()[2]) > 300
