"""The delivery kernels (csrc/tetra_rx_out.hip: k_out_count, k_out_layout, k_out_write, k_out_ext_layout, k_out_ext_write) on PLANTED
rows, through the public entry over caller rows (include/ext/tetra_rx_out_rows.h), against the delivery numpy makes of the same rows from
the documented layout (tests/rx_out_reference.py).  The chain's synthetic IQ cannot choose which rows fail their CRC; here every tile's
staging shift, every keep pattern at the tile and wavefront edges, the row-count clamps and a layout scan of several tiles per thread are
chosen.  Every comparison is on the whole destination, prefilled with a sentinel, a 256-byte guard in front and 4096 bytes behind it: the
written bytes are numpy's, every other byte is still the sentinel.  Everything is bytes: every comparison is exact."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import rx_out_reference as X
from tests.chain_host import noisy_batch as _noisy_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "ext", "tetra_rx_out_rows.h")
ARG, HIP, SIZE, ALIGN = -1, -4, -6, -7
FLAGS = (0, X.PACKED, X.CRC_GOOD, X.PACKED | X.CRC_GOOD)
GUARD, SLACK = 256, 4096
CALL = 0x1122334455                              # a call index that needs its 64 bits

# the residue case: 17 full tiles and a partial one of the kind looked at, a few rows of garbage behind them
RES_ROWS = 17 * X.TILE + 77
RES_MAX = RES_ROWS + 11
RES_OTHER = (150, 3, 129, 0, 260, 64)            # rows of the kinds not looked at (rotated by the kind looked at)
# the residues of 16 bytes a tile's type-1 rows can start at under TETRA_RX_OUT_CRC_GOOD: row_bytes * (kept rows before it) mod 16
REACHABLE = {(k, 0): {0, 4, 8, 12} for k in (0, 2, 3, 4, 5)}
REACHABLE.update({(1, 0): set(range(0, 16, 2)), (5, 1): set(range(0, 16, 2)), (1, 1): {0, 4, 8, 12}, (0, 1): {0, 8}, (2, 1): {0}, (3, 1): {0}, (4, 1): {0}})
NS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
NS_EXTRAS = (127, 128, 129, 256, 257)
EXTRAS = (1, 2, 4, 7)


@functools.lru_cache(None)
def pool(alloc_rows, seed=77):
    """six kinds' planted arrays of alloc_rows rows each, the last 7 garbage in every byte, made once per size and never changed"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(6):
        p = X.plant(rng, k, alloc_rows, garbage_rows=7)
        for v in p.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        out.append(p)
    return tuple(out)


def residue_case(kind, rng):
    """all six kinds in one launch: `kind` with the residue pattern, the others short with random verdicts"""
    return [X.with_keep(rng, p, X.residue_keep(RES_ROWS) if k == kind else rng.random(RES_OTHER[(k + kind) % 6]) < 0.6) for k, p in enumerate(pool(RES_MAX))]


def pattern_names():
    return list(X.keep_patterns(1)) + ["first of the second wave", "a tile dropped between two kept"]


def keep_pattern(name, n):
    if name == "first of the second wave":       # per tile, only lane 0 of its second wavefront
        keep = np.zeros(n, bool)
        keep[64::X.TILE] = True
        return keep
    if name == "a tile dropped between two kept":
        keep = np.ones(n, bool)
        keep[X.TILE: 2 * X.TILE] = False
        return keep
    return X.keep_patterns(n)[name] != 0


def pattern_case(n, first, rng, max_rows):
    """all six kinds with n rows; kind k takes pattern first + k of the six, so that each launch holds them all"""
    names = pattern_names()
    return [X.with_keep(rng, p, keep_pattern(names[(first + k) % len(names)], n)) for k, p in enumerate(pool(max_rows))]


# ---------------------------------------------------------------------------------------------------------------- CPU: ABI

def _decls():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    src = "\n".join(line for line in src.split("\n") if not line.lstrip().startswith("#"))
    return {m.group(2): (m.group(1), [a.strip() for a in " ".join(m.group(3).split()).split(",")])
            for m in re.finditer(r"\b(int|size_t)\s+(tetra_\w+)\s*\(([^()]*)\)\s*;", src)}


def test_rx_out_rows_header_is_exported_and_bound(pkg):
    """The two functions include/ext/tetra_rx_out_rows.h declares are the binding's RX_OUT_ROWS_EXPORTS, exported by the library, bound
    with the declared number of parameters and the declared width of every 64-bit, size_t and pointer parameter; the header compiles as
    C99 and C++11 (tests/test_abi.py's rule for include/*.h); no other header's list holds them."""
    R = pkg.rx_binding
    decls = _decls()
    assert list(decls) == ["tetra_rx_out_rows_workspace_bytes", "tetra_rx_out_write_rows_device"] == R.RX_OUT_ROWS_EXPORTS == list(R.OUT_ROWS_ABI)
    assert not set(decls) & (set(R.RX_OUT_EXPORTS) | set(R.RX_EXPORTS) | set(R.RX_OUT_EXT_EXPORTS))
    L = pkg.load_library()
    R._lib()
    wide = {"size_t": C.c_size_t, "uint64_t": C.c_uint64, "int64_t": C.c_int64}
    for name, (ret, params) in decls.items():
        fn = getattr(L, name)
        restype, argtypes = R.OUT_ROWS_ABI[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes) and len(argtypes) == len(params), name
        assert restype is (C.c_size_t if ret == "size_t" else C.c_int), name
        for decl, ct in zip(params, argtypes):
            ctype = decl.rsplit(" ", 1)[0].replace("const ", "").strip()
            if "*" in decl:
                assert C.sizeof(ct) == C.sizeof(C.c_void_p) and ct not in (C.c_int64, C.c_uint64, C.c_size_t), (name, decl)
            else:
                assert C.sizeof(ct) == C.sizeof(wide.get(ctype, C.c_int)) and (ctype in wide) == (ct is not C.c_int), (name, decl)
    assert len(decls["tetra_rx_out_write_rows_device"][1]) == 11
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", lang, HDR], check=True)


def test_rx_out_rows_struct_layout_matches_header(pkg):
    R = pkg.rx_binding
    T = "tetra_rx_out_rows_t"
    exprs = ["sizeof(%s)" % T] + ["offsetof(%s, %s)" % (T, f) for f, _ in R.OutRows._fields_] + ["sizeof(tetra_rx_block_t)", "TETRA_RX_N_KINDS"]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "ext/tetra_rx_out_rows.h"\nint main(void){' +
            "".join('printf("%%llu\\n", (unsigned long long)(%s));' % e for e in exprs) + "return 0;}\n")
    with tempfile.TemporaryDirectory() as td:
        cfile, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(cfile, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)
        v = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert v == [C.sizeof(R.OutRows)] + [getattr(R.OutRows, f).offset for f, _ in R.OutRows._fields_] + [R.BLOCK_DTYPE.itemsize, R.N_KINDS]
    assert C.sizeof(R.OutRows) == 56 and R.BLOCK_DTYPE.itemsize == 24
    # host only: the workspace is the tile counts plus the two layouts
    L = R._lib()
    sizes = [R.out_rows_workspace_bytes(n) for n in (1, 128, 129, 66000)]
    assert R.out_rows_workspace_bytes(0) == 0 == R.out_rows_workspace_bytes(-5)
    assert sizes[0] == sizes[1] and all(s % 16 == 0 for s in sizes)                              # 6 ints a tile, on 16 bytes
    assert [s - sizes[1] for s in sizes[2:]] == [X.a16(24 * t) - X.a16(24) for t in (2, (66000 + 127) // 128)]
    assert L.tetra_rx_out_write_rows_device(None, 1, 1, 0, 0, 0, None, 0, None, 0, None) == ARG


# ---------------------------------------------------------------------------------------------------------------- CPU: the reference

def test_numpy_delivery_is_what_the_host_readers_read(pkg):
    """tests/rx_out_reference.expected_delivery through the library's own readers (no GPU): per kind the labels and type-1 rows are the
    planted rows' [keep], the packed rows unpack to them, the columns are column[keep]; garbage behind the type-1 bits does not leak."""
    R = pkg.rx_binding
    rng = np.random.default_rng(2)
    kinds = pattern_case(257, 2, rng, 300)
    max_rows = 280
    kinds[3] = dict(kinds[3], n_rows=max_rows + 5)
    kinds[4] = dict(kinds[4], n_rows=-3)
    for flags in FLAGS:
        for extras in (0, 7, 2):
            buf, classic, total, kept = X.expected_delivery(R, kinds, max_rows, flags, CALL, extras)
            assert len(buf) == total and (extras != 0) == (total > classic)
            hd, got = R.view_delivery(buf)
            assert hd.bytes == classic and hd.call == CALL and hd.flags == flags and hd.status == 0
            if extras:
                ex, cols, chans = R.view_delivery_ext(buf)
                assert ex.bytes == total and ex.n_channels == 0 and ex.call == CALL and all(v is None for v in chans.values())
                assert ex.extras == extras and [ex.cell_offset, ex.sync_state_offset, ex.sync_misses_offset, ex.link_offset] == [0] * 4
            for i, rows in enumerate(kinds):
                k = rows["kind"]
                n_dec = X.clamp(rows["n_rows"], max_rows)
                keep = rows["ok"][:n_dec] != 0 if flags & X.CRC_GOOD else np.ones(n_dec, bool)
                assert hd.kinds[i].n_rows_decoded == n_dec == {3: max_rows, 4: 0}.get(k, 257), (flags, k)
                b, t = got[k]
                assert b.tobytes() == rows["blocks"][:n_dec][keep].tobytes(), (flags, k)
                if flags & X.PACKED:
                    assert t.shape[1] == X.PACKED_BYTES[k] and (np.unpackbits(t, axis=1)[:, X.TYPE1[k]:] == 0).all()
                    t = R.unpack_bits(t, X.TYPE1[k])
                assert np.array_equal(t, rows["type2"][:n_dec, :X.TYPE1[k]][keep]), (flags, k)
                if extras:
                    want = dict(biterr=rows["biterr"], rank=rows["rank"], aach_dist=rows["type2"][:, 30])
                    for c, name in enumerate(("biterr", "rank", "aach_dist")):
                        has = bool(extras & (1 << c)) and (c == 2) == (k == R.KIND_BBK)
                        assert (cols[k][name] is not None) == has, (flags, extras, k, name)
                        assert not has or np.array_equal(cols[k][name], want[name][:n_dec][keep]), (flags, extras, k, name)
    # a delivery that does not fit: the header alone, with the total
    buf, classic, total, _ = X.expected_delivery(R, kinds, max_rows, 0, CALL, 7, size=9000, capacity=classic)
    hd = R.OutHeader.from_buffer_copy(buf[:224].tobytes())
    assert hd.status == SIZE and hd.bytes == total > classic and (buf[224:] == X.SENTINEL).all()


def test_residue_pattern_reaches_every_shift(pkg):
    """The precondition of test_gpu_rows_residues, from the reference layout alone (no GPU, no library): under CRC_GOOD the tiles of the
    kind looked at start their type-1 rows at EVERY residue of 16 bytes that kind and packing can reach (REACHABLE: row_bytes * kept
    rows mod 16) and their labels at both word parities; without CRC_GOOD every tile starts at shift 0.  The dropped rows include lanes
    0 and 63 of both wavefronts."""
    R = pkg.rx_binding                           # (its ctypes mirror of the header serialises the reference's; no library call)
    keep = X.residue_keep(RES_ROWS)
    dropped = {int(i) % X.TILE for i in np.flatnonzero(~keep)}
    assert {0, 63, 64, 127} <= dropped and RES_ROWS % X.TILE and RES_ROWS // X.TILE == 17
    assert [int((~keep[t0: t0 + X.TILE]).sum()) for t0 in range(0, RES_ROWS, X.TILE)] == [1 + j % 3 for j in range(18)]
    for kind in range(6):
        kinds = residue_case(kind, np.random.default_rng(100 + kind))
        for packed in (0, 1):
            sh = X.tile_shifts(R, kinds, RES_MAX, X.CRC_GOOD | packed, kind)
            assert len(sh) == 18
            assert {b for b, _ in sh} == REACHABLE[(kind, packed)], (kind, packed, sorted({b for b, _ in sh}))
            assert {s for _, s in sh} == {0, 1}, (kind, packed)
            assert set(X.tile_shifts(R, kinds, RES_MAX, packed, kind)) == {(0, 0)}, (kind, packed)


# ---------------------------------------------------------------------------------------------------------------- GPU

class Gpu:
    """Planted rows on the device and launches over them.  The planted arrays of a pool are uploaded once; verdicts and row counts go
    up per launch; the workspace is filled with junk before every launch (its contents must not matter)."""

    def __init__(self, pkg):
        import torch
        self.torch, self.R, self.dev = torch, pkg.rx_binding, torch.device("cuda", 0)
        self.static, self.ws = {}, None

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def rows(self, r):
        key = id(r["type2"])
        if key not in self.static:
            self.static[key] = (r["type2"], {f: self.up(r[f]) for f in ("type2", "blocks", "biterr", "rank")})      # (the array is kept: its id stays its own)
        d = dict(self.static[key][1], kind=r["kind"], stride=r["stride"], crc_ok=self.up(r["ok"]), n_rows=self.up(np.array([r["n_rows"]], np.int32)))
        return d

    def workspace(self, max_rows):
        n = self.R.out_rows_workspace_bytes(max_rows)
        if self.ws is None or self.ws.numel() < n:
            self.ws = self.torch.empty(n, dtype=self.torch.uint8, device=self.dev)
        self.ws.fill_(0x3B)
        return self.ws[:n]

    def run(self, kinds, max_rows, flags, extras=0, capacity=None, size=None, stream=None, ws=None):
        """-> (guard + destination as numpy after the launch, its expectation, classic bytes, total bytes)"""
        exp, classic, total, _ = X.expected_delivery(self.R, kinds, max_rows, flags, CALL, extras, size=size, capacity=capacity)
        if size is None:
            exp = np.concatenate([exp, np.full(SLACK, X.SENTINEL, np.uint8)])
        exp = np.concatenate([np.full(GUARD, X.SENTINEL, np.uint8), exp])
        big = self.torch.full((len(exp),), X.SENTINEL, dtype=self.torch.uint8, device=self.dev)
        d = [self.rows(r) for r in kinds]
        self.R.out_write_rows(d, max_rows, big[GUARD:], self.workspace(max_rows) if ws is None else ws, packed=bool(flags & X.PACKED),
                              crc_good_only=bool(flags & X.CRC_GOOD), row_extras=extras, call_index=CALL, capacity=capacity, stream=stream)
        self.torch.cuda.synchronize()
        return big.cpu().numpy(), exp, classic, total


@pytest.fixture(scope="module")
def gpu(pkg):
    return Gpu(pkg)


def same(got, exp, ctx):
    if not np.array_equal(got, exp):
        i = np.flatnonzero(got != exp)
        raise AssertionError((ctx, "bytes that differ: %d, first at %s (destination offset %d): got %s, expected %s" %
                              (len(i), i[:6].tolist(), int(i[0]) - GUARD, got[i[:6]].tolist(), exp[i[:6]].tolist())))


def check(gpu, kinds, max_rows, flags, extras, ctx):
    got, exp, classic, total = gpu.run(kinds, max_rows, flags, extras)
    same(got, exp, ctx + (flags, extras))
    return got, classic, total


@pytest.mark.gpu
@pytest.mark.parametrize("kind", range(6))
def test_gpu_rows_residues(pkg, gpu, kind):
    """(a), and (e) on it: tiles whose staging shifts take every reachable value (test_residue_pattern_reaches_every_shift)."""
    kinds = residue_case(kind, np.random.default_rng(100 + kind))
    for flags in FLAGS:
        plain, classic, _ = check(gpu, kinds, RES_MAX, flags, 0, ("residues", kind))
        for extras in EXTRAS:
            got, c2, total = check(gpu, kinds, RES_MAX, flags, extras, ("residues", kind))
            assert c2 == classic and got[:GUARD + classic].tobytes() == plain[:GUARD + classic].tobytes() and total >= X.a16(classic) + 256


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_gpu_rows_keep_patterns(pkg, gpu, n):
    """(b), and (e) on it: every keep pattern at every tile and wavefront edge; the six kinds of a launch hold the six patterns."""
    max_rows = 257 + 7
    for first in range(len(pattern_names())):
        kinds = pattern_case(n, first, np.random.default_rng(1000 * n + first), max_rows)
        for flags in FLAGS:
            plain, classic, _ = check(gpu, kinds, max_rows, flags, 0, ("patterns", n, first))
            for extras in EXTRAS if n in NS_EXTRAS else ():
                got, c2, _ = check(gpu, kinds, max_rows, flags, extras, ("patterns", n, first))
                assert c2 == classic and got[:GUARD + classic].tobytes() == plain[:GUARD + classic].tobytes()
    # the exact row limit: n rows with max_rows = n (the tile count is taken from max_rows)
    if n:
        kinds = pattern_case(n, 2, np.random.default_rng(n), max_rows)
        for flags in FLAGS:
            check(gpu, kinds, n, flags, 7, ("patterns, max_rows = n", n))


@pytest.mark.gpu
def test_gpu_rows_row_count_clamps(pkg, gpu):
    """(c): counts above max_rows and below 0, tiny kinds beside a large one, a kinds subset that starts above SB1."""
    R = pkg.rx_binding
    rng = np.random.default_rng(31)
    p = pool(RES_MAX)
    max_rows = 1000
    for flags in FLAGS:
        for extras in (0, 7):
            over = [X.with_keep(rng, p[k], rng.random(max_rows) < 0.5, n_rows=max_rows + 5) for k in range(6)]
            got, classic, _ = check(gpu, over, max_rows, flags, extras, ("above max_rows",))
            hd = R.OutHeader.from_buffer_copy(got[GUARD: GUARD + 224].tobytes())
            assert [e.n_rows_decoded for e in hd.kinds] == [max_rows] * 6
            under = [X.with_keep(rng, p[k], rng.random(300) < 0.5, n_rows=-3 if k % 2 else 300) for k in range(6)]
            got, classic, _ = check(gpu, under, max_rows, flags, extras, ("below 0",))
            hd = R.OutHeader.from_buffer_copy(got[GUARD: GUARD + 224].tobytes())
            assert [e.n_rows_decoded for e in hd.kinds] == [300, 0] * 3 and [e.n_rows for e in hd.kinds][1::2] == [0] * 3
            mix = [X.with_keep(rng, p[k], rng.random(n) < 0.7) for k, n in enumerate((0, 1, 128, 2000, 128, 1))]
            check(gpu, mix, RES_MAX, flags, extras, ("mix",))
            allk = [X.with_keep(rng, p[k], np.ones(n, bool)) for k, n in enumerate((128, 0, 1, 128, 0, 2000))]
            check(gpu, allk, RES_MAX, flags, extras, ("mix, every row kept",))
            for sub in ((2, 5), (1,), (3, 4, 5), (5,)):
                check(gpu, [X.with_keep(rng, p[k], rng.random(200 + k) < 0.7) for k in sub], max_rows, flags, extras, ("subset", sub))


BIG = {1: 65537 + 129, 0: 32768 + 129, 2: 0, 3: 1, 4: 129, 5: 300}      # (d): BBK 3 tiles per scanning thread, SB1 2


@pytest.mark.gpu
def test_gpu_rows_scan_of_several_tiles_per_thread(pkg, gpu):
    """(d): the layout scan (compact_core::scan_counts, 256 threads) with 3 and 2 tiles per thread and one tile or none for the other
    kinds, CRC-good only, both packings: random verdicts at 70 %, and once with the whole run of tiles of one scanning thread empty (and
    of the last one that has tiles).  Each kind's arrays hold only its own rows and a few more: rows from *n_rows on are never read."""
    rng = np.random.default_rng(41)
    max_rows = BIG[1] + 3
    planted = [X.plant(rng, k, BIG[k] + 3, garbage_rows=3) for k in range(6)]
    tiles = {k: -(-BIG[k] // X.TILE) for k in BIG}
    assert -(-tiles[1] // 256) == 3 and -(-tiles[0] // 256) == 2
    random = [X.with_keep(rng, planted[k], rng.random(BIG[k]) < 0.7) for k in range(6)]
    empty = []
    for k in range(6):
        keep = rng.random(BIG[k]) < 0.7
        if k == 1:
            keep[3 * 10 * X.TILE: 3 * 11 * X.TILE] = False        # thread 10's tiles 30..32
            keep[3 * 170 * X.TILE:] = False                       # the last two threads with tiles (170: 510..512, 171: the partial 513)
        if k == 0:
            keep[2 * 5 * X.TILE: 2 * 6 * X.TILE] = False          # thread 5's tiles 10, 11
        empty.append(X.with_keep(rng, planted[k], keep))
    for name, kinds in (("random", random), ("empty runs", empty)):
        for flags in (X.CRC_GOOD, X.CRC_GOOD | X.PACKED):
            check(gpu, kinds, max_rows, flags, 0, ("scan", name))
    check(gpu, random, max_rows, X.CRC_GOOD, 7, ("scan", "random"))


@pytest.mark.gpu
def test_gpu_rows_capacity(pkg, gpu):
    """(f): exactly the bytes needed are enough; one byte less leaves the classic header alone (TETRA_ERR_SIZE, bytes = the total) and
    the sentinel everywhere else -- classic and extended; and one delivery into tetra_rx_out_host_alloc memory."""
    R = pkg.rx_binding
    rng = np.random.default_rng(51)
    kinds = pattern_case(257, 1, rng, 257 + 7)
    for flags in FLAGS:
        for extras in (0, 7, 4):
            _, _, classic, total = gpu.run(kinds, 264, flags, extras)
            for cap in (total, total - 1) + ((classic, classic - 1) if extras else ()):
                got, exp, _, _ = gpu.run(kinds, 264, flags, extras, capacity=cap, size=total + SLACK)
                same(got, exp, ("capacity", flags, extras, cap))
                hd = R.OutHeader.from_buffer_copy(got[GUARD: GUARD + 224].tobytes())
                assert (hd.status, hd.bytes) == ((0, classic) if cap == total else (SIZE, total)), (flags, extras, cap)
                assert cap == total or (got[GUARD + 224:] == X.SENTINEL).all()
    # mapped host memory, the guard by offsetting into it
    exp, classic, total, _ = X.expected_delivery(R, kinds, 264, 3, CALL, 7)
    host = R.HostBuffer(GUARD + total + SLACK)
    host.array[:] = X.SENTINEL
    R.out_write_rows([gpu.rows(r) for r in kinds], 264, host.array[GUARD:], gpu.workspace(264), packed=True, crc_good_only=True, row_extras=7,
                     call_index=CALL)
    gpu.torch.cuda.synchronize()
    got = host.array.copy()
    host.close()
    same(got[GUARD: GUARD + total], exp, ("host memory",))
    assert (got[:GUARD] == X.SENTINEL).all() and (got[GUARD + total:] == X.SENTINEL).all()


@pytest.mark.gpu
def test_gpu_rows_statuses(pkg, gpu):
    """(g): every row of the header's status table that one GPU can produce (memory of another GPU, a missing device and a failed launch
    cannot be had here), none of which writes a byte; a NULL column of a kind that does not carry it is no error; two launches back to
    back on one stream with one workspace give two correct deliveries."""
    R = pkg.rx_binding
    L = R._lib()
    torch = gpu.torch
    rng = np.random.default_rng(61)
    p = pool(264)
    kinds = [X.with_keep(rng, p[k], rng.random(200) < 0.5) for k in (0, 1, 5)]
    d = [gpu.rows(r) for r in kinds]
    big = torch.full((GUARD + 65536,), X.SENTINEL, dtype=torch.uint8, device=gpu.dev)
    dst, cap = big.data_ptr() + GUARD, 65536
    ws = gpu.workspace(264)
    wsb = R.out_rows_workspace_bytes(264)
    pageable = np.full(65536, X.SENTINEL, np.uint8)

    def rc(arr=None, n_kinds=3, max_rows=264, flags=0, extras=0, dst=dst, cap=cap, wsp=ws.data_ptr(), wsb=wsb, edit=None, null_arr=False):
        arr = R.out_rows_arg(d) if arr is None else arr
        if edit:
            i, field, value = edit
            cur = getattr(arr[i], field)
            setattr(arr[i], field, value(cur) if callable(value) else value)
        return L.tetra_rx_out_write_rows_device(None if null_arr else arr, n_kinds, max_rows, flags, extras, CALL, dst, cap, wsp, wsb, None)

    assert rc() == 0
    torch.cuda.synchronize()
    big.fill_(X.SENTINEL)
    table = [(ARG, dict(null_arr=True)), (ARG, dict(dst=None)), (ARG, dict(wsp=None)), (ARG, dict(dst=pageable.ctypes.data))]
    table += [(ARG, dict(n_kinds=v)) for v in (0, -1, 7)] + [(ARG, dict(max_rows=v)) for v in (0, -1)]
    table += [(ARG, dict(flags=v)) for v in (4, 8, -1)] + [(ARG, dict(extras=v)) for v in (8, 16, 32, 64, 128, 240, 247, 256, -1)]
    table += [(ARG, dict(edit=(1, "kind", v))) for v in (-1, 6, 0, 5, 7)]            # no kind, twice, not ascending
    table += [(ARG, dict(edit=(2, "kind", 1)))]
    table += [(ARG, dict(edit=(i, f, None))) for i in range(3) for f in ("d_type2", "d_crc_ok", "d_blocks", "d_n_rows")]
    table += [(ARG, dict(edit=(0, "type2_stride", v))) for v in (56, 63, 0, -80)] + [(ARG, dict(edit=(1, "type2_stride", v))) for v in (24, 31)]
    table += [(ARG, dict(edit=(2, "type2_stride", v))) for v in (264, 271)]
    table += [(ARG, dict(extras=e, edit=(i, f, None))) for e, f in ((1, "d_biterr"), (2, "d_rank"), (7, "d_biterr"), (7, "d_rank")) for i in (0, 2)]
    table += [(ALIGN, dict(dst=dst + o)) for o in (1, 4, 8)] + [(ALIGN, dict(wsp=ws.data_ptr() + 8, wsb=wsb))]
    table += [(ALIGN, dict(edit=(i, f, lambda v, o=o: v + o))) for i in (0, 1) for f, o in (("d_type2", 4), ("d_blocks", 4), ("d_crc_ok", 2), ("d_n_rows", 2),
                                                                                        ("d_biterr", 2), ("d_rank", 1))]
    table += [(ALIGN, dict(edit=(0, "type2_stride", 68))), (ALIGN, dict(edit=(2, "type2_stride", 284)))]
    table += [(SIZE, dict(cap=v)) for v in (0, 223)] + [(SIZE, dict(wsb=wsb - 1)), (SIZE, dict(wsb=0))]
    for want, kw in table:
        assert rc(**kw) == want, (want, {k: v for k, v in kw.items() if k != "edit"}, kw.get("edit", (None, None))[:2])
    torch.cuda.synchronize()
    assert (big.cpu().numpy() == X.SENTINEL).all() and (pageable == X.SENTINEL).all()
    # no error: the BBK without counts and ranks, the coded kinds' columns unasked for
    assert rc(extras=3, edit=(1, "d_biterr", None)) == 0 and rc(extras=3, edit=(1, "d_rank", None)) == 0
    assert rc(extras=4, edit=(0, "d_biterr", None)) == 0 and rc(extras=0, edit=(2, "d_rank", None)) == 0 and rc(cap=224) == 0
    torch.cuda.synchronize()
    # twice on one stream, one workspace, two buffers
    s = torch.cuda.Stream(gpu.dev)
    other = [X.with_keep(rng, p[k], rng.random(250) < 0.3) for k in range(6)]
    exps, bufs = [], []
    shared = gpu.workspace(264)
    torch.cuda.synchronize()
    for kk, flags, extras in ((kinds, X.CRC_GOOD, 7), (other, X.CRC_GOOD | X.PACKED, 3)):
        exp = X.expected_delivery(R, kk, 264, flags, CALL, extras)[0]
        exps.append(np.concatenate([np.full(GUARD, X.SENTINEL, np.uint8), exp, np.full(SLACK, X.SENTINEL, np.uint8)]))
        bufs.append((torch.full((len(exps[-1]),), X.SENTINEL, dtype=torch.uint8, device=gpu.dev), [gpu.rows(r) for r in kk], flags, extras))
    torch.cuda.synchronize()
    for b, dk, flags, extras in bufs:
        R.out_write_rows(dk, 264, b[GUARD:], shared, packed=bool(flags & X.PACKED), crc_good_only=True, row_extras=extras, call_index=CALL, stream=s)
    s.synchronize()
    for i, (b, _, _, _) in enumerate(bufs):
        same(b.cpu().numpy(), exps[i], ("back to back", i))


@pytest.mark.gpu
def test_gpu_rows_equal_the_chains_delivery(pkg, gpu, synth):
    """(h): one call of tests/test_rx_out.py's noisy batch (seed 9100) through the chain; its rows, fetched with the blocking fetches and
    planted through the entry, give the chain's own delivery byte for byte (the call index is passed in), for the four flag combinations
    -- and both are numpy's."""
    R = pkg.rx_binding
    Cn, nslots = 8, 72
    N = nslots * 510 // 2
    _, _, iq = _noisy_batch(synth, Cn, nslots, 2 * N, 9100)
    rx = pkg.RxChain(Cn, N)
    rx.process(iq[:, :N])
    rx.wait()
    rng = np.random.default_rng(71)
    kinds = []
    for k in range(6):
        b, t1 = rx.fetch(k)
        n = len(b)
        p = X.plant(rng, k, n + 3, garbage_rows=3)
        p["type2"][:n, :X.TYPE1[k]] = t1
        p["blocks"][:n] = np.frombuffer(b.tobytes(), np.uint8).reshape(n, 24)
        r = X.with_keep(rng, p, b["crc_ok"] != 0)
        r["ok"][:n] = b["crc_ok"]
        kinds.append(r)
    assert sum(r["n_rows"] for r in kinds) > 300 and sum(int((r["ok"][:r["n_rows"]] == 0).sum()) for r in kinds) > 0
    for flags in FLAGS:
        buf = R.HostBuffer(rx.out_bound(packed=bool(flags & 1), crc_good_only=bool(flags & 2)) + SLACK)
        buf.array[:] = X.SENTINEL
        d = rx.deliver(0, packed=bool(flags & 1), crc_good_only=bool(flags & 2), buf=buf)
        d.wait()
        nb = int(d.header.bytes)
        chain = buf.array[:nb].copy()
        assert d.header.call == 0 and (buf.array[nb:] == X.SENTINEL).all()
        buf.close()
        exp, classic, _, _ = X.expected_delivery(R, kinds, rx.max_rows, flags, 0)
        assert classic == nb, flags
        big = gpu.torch.full((GUARD + nb + SLACK,), X.SENTINEL, dtype=gpu.torch.uint8, device=gpu.dev)
        R.out_write_rows([gpu.rows(r) for r in kinds], rx.max_rows, big[GUARD:], gpu.workspace(rx.max_rows), packed=bool(flags & 1),
                         crc_good_only=bool(flags & 2), call_index=0)
        gpu.torch.cuda.synchronize()
        got = big.cpu().numpy()
        same(got[GUARD: GUARD + nb], chain, ("chain", flags))
        same(chain, exp, ("chain against numpy", flags))
        assert (got[:GUARD] == X.SENTINEL).all() and (got[GUARD + nb:] == X.SENTINEL).all()
    rx.close()
