"""The one-step delivery in plain numpy, from the documented layout alone (include/tetra_rx_out.h, include/ext/tetra_rx_out_ext.h): what
tests/test_rx_out_ext.py lays out by hand for the host readers, and what tests/test_rx_out_rows.py holds the delivery kernels against on
planted rows.  Nothing here calls the library; the ctypes mirrors of the two headers (rx_binding, passed in as R) only serialise them."""
import ctypes as C

import numpy as np

from tests.chain_host import PACKED_BYTES, TYPE1_BITS as TYPE1          # per kind: type-1 bits, and the bytes they pack into

STRIDE = [80, 32, 144, 144, 144, 288]            # the chain's type-2 row strides (tetra_rx_rows_device)
CHAN_BYTES = [40, 16, 4, 24]
SENTINEL = 0xA5
TILE = 128                                       # rows per workgroup of the delivery kernels
KIND_BBK = 1
PACKED, CRC_GOOD = 1, 2
AACH_DIST_BYTE = 30


def a16(x):
    return (x + 15) // 16 * 16


def row_bytes(kind, flags):
    return PACKED_BYTES[kind] if flags & PACKED else TYPE1[kind]


def keep_patterns(n):
    last_of_tile = np.zeros(n, np.int32)
    last_of_tile[127::128] = 1
    if n:
        last_of_tile[n - 1] = 1
    every_second = (np.arange(n) % 2).astype(np.int32)
    return {"all": np.ones(n, np.int32), "none": np.zeros(n, np.int32), "every second": every_second, "last of a tile": last_of_tile}


def build_ext_delivery(R, rows, flags, extras, n_channels, rng):
    """An extended delivery laid out by hand as include/ext/tetra_rx_out_ext.h documents it, behind test_rx_out's classic one ->
    (buffer, classic rows, {kind: [biterr, rank, dist] (None = absent)}, [cell, sync, misses, link] as bytes (None = absent),
    section boundaries)."""
    from tests.test_rx_out import _build_delivery
    classic, want = _build_delivery(R, rows, flags, rng)
    kinds = sorted(rows)
    ex = R.OutExtHeader()
    ex.magic, ex.call, ex.n_channels, ex.n_kinds = R.OUT_EXT_MAGIC, 41, n_channels, len(kinds)
    at = a16(len(classic))
    end = at + C.sizeof(R.OutExtHeader)
    got, cols, parts, bounds = extras & R.EXT_CHAN_ALL, {}, [], [len(classic), at, end]
    for i, k in enumerate(kinds):
        n = rows[k]
        e = ex.kinds[i]
        e.kind, e.n_rows = k, n
        cols[k] = [None, None, None]
        for c, (field, dtype, hi) in enumerate((("biterr_offset", "<u4", 2 ** 32), ("rank_offset", "<i4", 9), ("aach_dist_offset", "u1", 256))):
            if not extras & (1 << c) or (c == 2) != (k == R.KIND_BBK):
                continue
            off = a16(end)
            setattr(e, field, off)
            v = rng.integers(-1 if c == 1 else 0, hi, n).astype(dtype)
            cols[k][c] = v
            parts.append((off, v.tobytes()))
            end = off + v.nbytes
            bounds.append(end)
            got |= 1 << c
    tabs = [None] * 4
    for t, field in enumerate(("cell_offset", "sync_state_offset", "sync_misses_offset", "link_offset")):
        if not extras & (R.EXT_CHAN_CELL << t):
            continue
        off = a16(end)
        setattr(ex, field, off)
        tabs[t] = rng.integers(0, 256, CHAN_BYTES[t] * n_channels).astype(np.uint8).tobytes()
        parts.append((off, tabs[t]))
        end = off + len(tabs[t])
        bounds.append(end)
    ex.extras, ex.bytes = got, end
    buf = np.zeros(end, np.uint8)
    buf[:len(classic)] = classic
    buf[at: at + C.sizeof(R.OutExtHeader)] = np.frombuffer(bytes(ex), np.uint8)
    for off, b in parts:
        buf[off: off + len(b)] = np.frombuffer(b, np.uint8)
    return buf, want, cols, tabs, sorted(set(bounds))


# ---- planted rows and the delivery numpy makes of them ------------------------------------------------------------------------------

OK_VALUES = np.array([1, 1, 2, -1, -7, 255, 256, 2 ** 31 - 1, -2 ** 31], np.int64)      # what "crc_ok != 0" has to hold for


def clamp(n, max_rows):
    return min(max(int(n), 0), int(max_rows))


def plant(rng, kind, alloc_rows, stride=None, garbage_rows=0):
    """One kind's planted arrays of alloc_rows rows: random 24-byte labels (their own crc_ok field is random too), type-2 rows whose
    first type1_bits bytes are random 0 / 1 and whose every other byte is garbage 0..255 -- as is every byte of the last garbage_rows
    rows, which no case counts among its decoded rows --, random counts, ranks.  The verdicts (`ok`) and the row count are set per case
    (with_keep)."""
    stride = STRIDE[kind] if stride is None else stride
    nb, good = TYPE1[kind], alloc_rows - garbage_rows
    t2 = rng.integers(0, 256, (alloc_rows, stride)).astype(np.uint8)
    t2[:good, :nb] = rng.integers(0, 2, (good, nb))
    return dict(kind=kind, stride=stride, type2=t2, blocks=rng.integers(0, 256, (alloc_rows, 24)).astype(np.uint8),
                biterr=rng.integers(0, 2 ** 32, alloc_rows, dtype=np.uint64).astype(np.uint32),
                rank=rng.integers(-2 ** 31, 2 ** 31, alloc_rows).astype(np.int32))


def with_keep(rng, rows, keep, n_rows=None):
    """rows (plant) with the verdict array for `keep` (bool per decoded row): 0 where a row is dropped, a non-zero value (negative ones
    and values above 1 included) where it is kept, non-zero past the decoded rows; and the row count the device is told (n_rows,
    default len(keep)), which may lie outside 0..max_rows."""
    keep = np.asarray(keep).astype(bool)
    alloc = len(rows["type2"])
    assert len(keep) <= alloc
    ok = rng.choice(OK_VALUES, alloc)
    ok[:len(keep)][~keep] = 0
    return dict(rows, ok=ok.astype(np.int32), n_rows=len(keep) if n_rows is None else int(n_rows))


def type1_rows(rows, sel, flags):
    """type-1 rows of the selected rows as the delivery holds them: a byte per bit, or packed with zero padding"""
    bits = rows["type2"][sel][:, :TYPE1[rows["kind"]]]
    return np.packbits(bits, axis=1) if flags & PACKED else bits


def expected_delivery(R, kinds, max_rows, flags, call, extras=0, size=None, capacity=None):
    """The bytes a delivery of the planted `kinds` (ascending, each from with_keep) leaves in a destination of `size` bytes prefilled with
    SENTINEL, written from the documented layout alone -> (uint8 [size], classic bytes, total bytes, {kind: kept row indices}).
    capacity (default size): a delivery that needs more leaves only its classic header, status TETRA_ERR_SIZE, bytes = the total."""
    hd = R.OutHeader()
    hd.magic, hd.status, hd.flags, hd.n_kinds, hd.call = R.OUT_MAGIC, 0, flags, len(kinds), call
    off, sections, kept = C.sizeof(R.OutHeader), [], {}
    for i, rows in enumerate(kinds):
        k = rows["kind"]
        n_dec = clamp(rows["n_rows"], max_rows)
        sel = np.flatnonzero(rows["ok"][:n_dec] != 0) if flags & CRC_GOOD else np.arange(n_dec)
        kept[k] = sel
        e = hd.kinds[i]
        e.kind, e.n_rows, e.n_rows_decoded, e.row_bytes = k, len(sel), n_dec, row_bytes(k, flags)
        e.blocks_offset = a16(off)
        e.bits_offset = a16(e.blocks_offset + 24 * len(sel))
        off = e.bits_offset + e.row_bytes * len(sel)
        t1 = type1_rows(rows, sel, flags)
        assert t1.shape == (len(sel), e.row_bytes)
        sections += [(int(e.blocks_offset), rows["blocks"][sel].tobytes()), (int(e.bits_offset), np.ascontiguousarray(t1).tobytes())]
    hd.bytes = classic = total = off
    if extras:
        ex = R.OutExtHeader()
        ex.magic, ex.call, ex.n_channels, ex.n_kinds = R.OUT_EXT_MAGIC, call, 0, len(kinds)
        at = a16(classic)
        end, got = at + C.sizeof(R.OutExtHeader), 0
        for i, rows in enumerate(kinds):
            k, sel = rows["kind"], kept[rows["kind"]]
            e = ex.kinds[i]
            e.kind, e.n_rows = k, len(sel)
            cols = (("biterr_offset", rows["biterr"]), ("rank_offset", rows["rank"]), ("aach_dist_offset", rows["type2"][:, AACH_DIST_BYTE]))
            for c, (field, col) in enumerate(cols):
                if not extras & (1 << c) or (c == 2) != (k == KIND_BBK):
                    continue
                o = a16(end)
                setattr(e, field, o)
                b = np.ascontiguousarray(col[sel]).tobytes()
                sections.append((o, b))
                end = o + len(b)
                got |= 1 << c
        ex.extras, ex.bytes = got, end
        sections.append((at, bytes(ex)))
        total = end
    size = total if size is None else size
    capacity = size if capacity is None else capacity
    buf = np.full(size, SENTINEL, np.uint8)
    if total > capacity:
        hd.status, hd.bytes, sections = -6, total, []
    for o, b in [(0, bytes(hd))] + sections:
        buf[o: o + len(b)] = np.frombuffer(b, np.uint8)
    return buf, classic, total, kept


def tile_shifts(R, kinds, max_rows, flags, kind):
    """Per tile of `kind` that keeps a row, from the reference layout: (bshift, lshift) = the first output byte of the tile's type-1
    rows mod 16 and the parity of its first label word -- the two shifts k_out_write stages a tile at."""
    buf, _, _, kept = expected_delivery(R, kinds, max_rows, flags, 0)
    hd = R.OutHeader.from_buffer_copy(buf[:C.sizeof(R.OutHeader)].tobytes())
    i = [rows["kind"] for rows in kinds].index(kind)
    e, sel, out = hd.kinds[i], kept[kind], []
    for t0 in range(0, e.n_rows_decoded, TILE):
        base = int(np.searchsorted(sel, t0))                 # kept rows before the tile (= t0 when every row is kept)
        if base < len(sel) and sel[base] < t0 + TILE:
            out.append((int(e.bits_offset + e.row_bytes * base) % 16, int(e.blocks_offset // 8 + 3 * base) % 2))
    return out


def residue_keep(n):
    """The keep pattern of the residue case: tile j drops 1 + (j % 3) rows, at positions that walk over the first and the last lane of
    each of the tile's two wavefronts (0, 63, 64, 127; folded into a partial last tile), so that the tiles' first output rows take
    every residue mod 16 and both parities."""
    keep = np.ones(n, bool)
    lanes = (0, 63, 64, 127)
    for j, t0 in enumerate(range(0, n, TILE)):
        rows = min(TILE, n - t0)
        for i in range(1 + j % 3):
            keep[t0 + lanes[(j + i) % 4] % rows] = False
    return keep
