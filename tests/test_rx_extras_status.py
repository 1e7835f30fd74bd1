"""The statuses of every reader of the receive chain's opt-in row extras and per-channel tables -- the blocking fetches and device views
(ext/tetra_biterr.h, ext/tetra_list.h, tetra_aach.h), the four per-channel getters (tetra_rx.h, ext/tetra_sync_tol.h, ext/tetra_biterr.h)
and the extended delivery's entries (ext/tetra_rx_out_ext.h) -- over the handle flags and kind selections that decide them, before the
first process call and after it.  The expectations are one literal table written from those headers; contents are other tests' business."""
import ctypes as C

import numpy as np
import pytest

OK, ARG, UNSUPPORTED, SIZE = 0, -1, -2, -6
ST = {"O": OK, "A": ARG, "U": UNSUPPORTED}
CN, MAX_SAMPLES = 2, 2000
NO_BBK = 0b100101                         # SB1, SB2, SCH/F: neither the AACH nor the normal bursts' blocks are decoded
EXTRA_BITS = (1, 2, 4, 16, 32, 64, 128)   # ROW_BITERR, ROW_LIST_RANK, ROW_AACH_DIST, CHAN_CELL, CHAN_SYNC_STATE, CHAN_SYNC_MISSES, CHAN_LINK

# One row per handle: (flag names, kinds) -> a letter per question, O = TETRA_OK, U = TETRA_ERR_UNSUPPORTED, A = TETRA_ERR_ARG.
#   biterr / rank   per kind SB1 BBK SB2 NDB1 NDB2 SCH/F: "the handle was created without the flag, for TETRA_RX_KIND_BBK, or for a kind the
#                   handle does not decode" is unsupported; the device views answer the same question
#   dist            "created without the flag or does not decode BBK"
#   getters         cell, sync state, sync misses, link: only the link figures need a flag (the misses are 0 under the reference's rule)
#   extras          per bit of EXTRA_BITS through tetra_rx_out_bound_ext and tetra_rx_out_enqueue_ext: "an extra whose flag the handle was
#                   created without"; the miss counters need TETRA_RX_FLAG_SYNC_TOLERANT or a tolerance set; the distance a handle that
#                   decodes BBK
#   snapshot        the same bits through tetra_rx_out_set_snapshot: a row extra is "a bit outside TETRA_RX_OUT_EXT_CHAN_ALL"
TABLE = [
    # flags,                                       kinds,  biterr,   rank,     dist, getters, extras,    snapshot
    ((),                                           0,      "UUUUUU", "UUUUUU", "U",  "OOOU",  "UUUOOUU", "AAAOOUU"),
    (("BITERR",),                                  0,      "OUOOOO", "UUUUUU", "U",  "OOOO",  "OUUOOUO", "AAAOOUO"),
    (("LIST",),                                    0,      "UUUUUU", "OUOOOO", "U",  "OOOU",  "UOUOOUU", "AAAOOUU"),
    (("AACH_RM3014",),                             0,      "UUUUUU", "UUUUUU", "O",  "OOOU",  "UUOOOUU", "AAAOOUU"),
    (("SYNC_TOLERANT",),                           0,      "UUUUUU", "UUUUUU", "U",  "OOOU",  "UUUOOOU", "AAAOOOU"),
    (("BITERR", "LIST", "AACH_RM3014", "SYNC_TOLERANT"), 0, "OUOOOO", "OUOOOO", "O", "OOOO",  "OOOOOOO", "AAAOOOO"),
    ((),                                           NO_BBK, "UUUUUU", "UUUUUU", "U",  "OOOU",  "UUUOOUU", "AAAOOUU"),
    (("BITERR",),                                  NO_BBK, "OUOUUO", "UUUUUU", "U",  "OOOO",  "OUUOOUO", "AAAOOUO"),
    (("LIST",),                                    NO_BBK, "UUUUUU", "OUOUUO", "U",  "OOOU",  "UOUOOUU", "AAAOOUU"),
    (("AACH_RM3014",),                             NO_BBK, "UUUUUU", "UUUUUU", "U",  "OOOU",  "UUUOOUU", "AAAOOUU"),
    (("SYNC_TOLERANT",),                           NO_BBK, "UUUUUU", "UUUUUU", "U",  "OOOU",  "UUUOOOU", "AAAOOOU"),
    (("BITERR", "LIST", "AACH_RM3014", "SYNC_TOLERANT"), NO_BBK, "OUOUUO", "OUOUUO", "U", "OOOO", "OOUOOOO", "AAAOOOO"),
]


@pytest.fixture(scope="module")
def noise():
    rng = np.random.default_rng(20)
    return (rng.normal(0, 1, (CN, MAX_SAMPLES)) + 1j * rng.normal(0, 1, (CN, MAX_SAMPLES))).astype(np.complex64)


@pytest.mark.gpu
@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s-%s" % ("+".join(r[0]) or "none", "all" if r[1] == 0 else "no_bbk"))
def test_gpu_rx_extras_statuses_are_the_headers(pkg, noise, row):
    flag_names, kinds, t_biterr, t_rank, t_dist, t_get, t_extras, t_snap = row
    R = pkg.rx_binding
    L = R._lib()
    rx = pkg.RxChain(CN, MAX_SAMPLES, kinds=kinds, flags=sum(getattr(R, "FLAG_" + f) for f in flag_names))
    h = rx._h
    n, nb, call = C.c_int(-1), C.c_uint64(0), C.c_int64(-1)
    configured = [k for k in range(R.N_KINDS) if kinds == 0 or kinds >> k & 1]
    every = sum(b for b, s in zip(EXTRA_BITS, t_extras) if s == "O")
    assert L.tetra_rx_out_bound_ext(h, 0, 0, every, C.byref(nb)) == OK
    buf = R.HostBuffer(nb.value)
    dst = C.c_void_p(buf.ptr)
    # (name, entry, kinds it is asked for, its letters, element type, device view)
    fetches = [("biterr", L.tetra_rx_fetch_biterr, range(R.N_KINDS), t_biterr, np.uint32, L.tetra_rx_biterr_device),
               ("rank", L.tetra_rx_fetch_list_rank, range(R.N_KINDS), t_rank, np.int32, L.tetra_rx_list_rank_device),
               ("dist", L.tetra_rx_fetch_aach_dist, (None,), t_dist, np.uint8, None)]
    getters = [(L.tetra_rx_get_cell, R.CellState), (L.tetra_rx_get_sync_state, R.BsyncState), (L.tetra_rx_get_sync_misses, C.c_int32),
               (L.tetra_rx_get_link, R.Link)]

    def readers(calls):
        for name, fetch, over, letters, dtype, device in fetches:
            for k, s in zip(over, letters):
                ka = () if k is None else (k,)
                ctx = (name, k, calls)
                rows = 0
                if s == "O" and calls:          # the rows the plain fetch counts are the rows this column has
                    assert L.tetra_rx_fetch(h, 0, R.KIND_BBK if k is None else k, None, None, 0, 0, C.byref(n)) == OK
                    rows = n.value
                n.value = -1
                assert fetch(h, 0, *ka, None, 0, C.byref(n)) == ST[s], ctx                       # a caller that only counts
                assert n.value == (rows if s == "O" else -1), ctx
                out = np.zeros(rows + 1, dtype)
                assert fetch(h, 0, *ka, out.ctypes.data, rows, C.byref(n)) == ST[s], ctx
                assert fetch(h, 1, *ka, out.ctypes.data, rows + 1, C.byref(n)) == ST[s] and (s != "O" or n.value == 0), ctx      # no previous call yet
                if s == "O" and rows:           # the capacity rule: one short with an output is refused, and still counts
                    n.value = -1
                    assert fetch(h, 0, *ka, out.ctypes.data, rows - 1, C.byref(n)) == SIZE and n.value == rows, ctx
                    assert fetch(h, 0, *ka, None, rows - 1, C.byref(n)) == OK and n.value == rows, ctx
                assert fetch(h, 0, *ka, out.ctypes.data, rows, None) == ARG and fetch(h, 2, *ka, None, 0, C.byref(n)) == ARG, ctx
                if device is not None:          # a view of a call that does not exist is an argument error, as tetra_rx_rows_device's
                    d = C.c_void_p()
                    assert device(h, 0, k, C.byref(d), None) == (ST[s] if s == "U" or calls else ARG), ctx
                    assert (d.value is not None) == (s == "O" and calls > 0), ctx
                    assert device(h, 1, k, C.byref(d), None) == (ST[s] if s == "U" else ARG), ctx
                    assert device(h, 0, k, None, None) == ARG and device(h, 0, R.N_KINDS, C.byref(d), None) == ARG, ctx
        for (get, elem), s in zip(getters, t_get):
            arr = (elem * (CN + 1))()
            assert get(h, 0, CN, arr) == ST[s] and get(h, CN, 0, arr) == ST[s] and get(h, 1, CN - 1, arr) == ST[s], (get.__name__, calls)
            # a range outside the channels is an argument error whatever the handle's flags
            assert get(h, 1, CN, arr) == ARG and get(h, 0, CN + 1, arr) == ARG and get(h, -1, 1, arr) == ARG and get(h, 0, CN, None) == ARG, (get.__name__, calls)
        if "SYNC_TOLERANT" not in flag_names:   # never tolerant: the getter answers zeros, the delivery has no such table
            assert not rx.sync_misses().any()
        for bit, s in zip(EXTRA_BITS, t_extras):
            assert L.tetra_rx_out_bound_ext(h, 0, 0, bit, C.byref(nb)) == ST[s], (bit, calls)
            assert L.tetra_rx_out_bound_ext(h, sum(1 << k for k in configured), R.OUT_PACKED, bit, C.byref(nb)) == ST[s], (bit, calls)
            # no call to deliver yet: an argument error, behind the question whether the handle has the extra at all
            want = ST[s] if s == "U" or calls else ARG
            assert L.tetra_rx_out_enqueue_ext(h, 0, 0, 0, bit, dst, buf.nbytes, C.byref(call)) == want, (bit, calls)
            if want == OK:
                assert L.tetra_rx_out_wait(h, call) == OK and R.OutHeader.from_buffer_copy(buf.array[:224].tobytes()).status == OK, (bit, calls)
            assert L.tetra_rx_out_enqueue_ext(h, 1, 0, 0, bit, dst, buf.nbytes, C.byref(call)) == (ST[s] if s == "U" else ARG), (bit, calls)
        for bit, s in zip(EXTRA_BITS, t_snap):
            assert L.tetra_rx_out_set_snapshot(h, bit) == ST[s], (bit, calls)
        assert L.tetra_rx_out_set_snapshot(h, every & R.EXT_CHAN_ALL) == OK       # armed for the call that follows

    readers(0)
    rx.process(noise)
    rx.wait()
    readers(1)
    rx.close()
    buf.close()
