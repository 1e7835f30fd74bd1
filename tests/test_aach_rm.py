"""The AACH decoded with its shortened (30,14) Reed-Muller code (include/tetra_aach.h; EN 300 392-2 8.2.3.2).

The encoder is pinned on the reference's own tetra_rm3014_compute (tests/golden/rm3014_codewords.npy, recorded by
tests/golden/gen_rm3014_golden.py); the reference has no decoder to hold to (lower_mac/tetra_rm3014.c:88-96 is a stub), so the decoder
is held to the code itself: d = 8, every error pattern of weight <= 3 corrected, every one of weight 4 refused, and a brute-force
nearest-codeword search over the golden codewords for random words.  CPU tests run the lane code built for the host
(tests/emul/rm3014_emul.cpp); GPU tests hold every entry point to that lane code word for word."""
import itertools
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
UNDEC = 0xFF
_PC16 = np.array([bin(v).count("1") for v in range(1 << 16)], np.uint8)


def popcount(x):
    x = np.asarray(x, np.uint32)
    return _PC16[x & 0xffff].astype(np.int32) + _PC16[x >> 16]


def golden():
    return np.load(os.path.join(HERE, "golden", "rm3014_codewords.npy"))


def patterns(weight):
    """every 30-bit error pattern of one weight"""
    if weight == 0:
        return np.zeros(1, np.uint32)
    return np.array([sum(1 << b for b in c) for c in itertools.combinations(range(30), weight)], np.uint32)


def np_rm3014_decode(words, code):
    """Bounded-distance decoding by brute force: the nearest of the 16 384 codewords if it is within distance 3, else the word."""
    words = np.asarray(words, np.uint32) & 0x3fffffff
    out, dist = words.copy(), np.full(words.size, UNDEC, np.uint8)
    for at in range(0, words.size, 256):
        w = words[at:at + 256]
        d = popcount(w[:, None] ^ code[None, :])
        j = d.argmin(axis=1)
        dm = d[np.arange(w.size), j]
        ok = dm <= 3
        out[at:at + 256][ok] = code[j[ok]]
        dist[at:at + 256][ok] = dm[ok]
    return out, dist


def bits_of(words):
    """30-bit words -> uint8 [n][30], first bit on air (bit 29) first"""
    return ((np.asarray(words, np.uint32)[:, None] >> (29 - np.arange(30))[None, :]) & 1).astype(np.uint8)


def words_of(bits):
    return (np.asarray(bits, np.uint32)[:, :30] << (29 - np.arange(30, dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)


def four_codewords():
    g = golden()
    rng = np.random.default_rng(3014)
    return [g[0], g[0x3fff], g[int(rng.integers(1, 0x3fff))], g[int(rng.integers(1, 0x3fff))]]


def primitive_cases():
    """The inputs of the CPU tests 2-4 and the clean codewords: (words, expected words, expected dist) from the code's definition."""
    g = golden()
    w, ew, ed = [], [], []
    for c in four_codewords():
        for k in range(4):
            p = patterns(k)
            w.append(c ^ p), ew.append(np.full(p.size, c, np.uint32)), ed.append(np.full(p.size, k, np.uint8))
    p4 = patterns(4)
    w.append(p4), ew.append(p4), ed.append(np.full(p4.size, UNDEC, np.uint8))
    w.append(g), ew.append(g), ed.append(np.zeros(g.size, np.uint8))
    return np.concatenate(w), np.concatenate(ew), np.concatenate(ed)


def random_words():
    return np.random.default_rng(30014).integers(0, 1 << 30, 4000, dtype=np.uint64).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------- CPU


def test_encoder_reproduces_the_reference_codewords_and_distance_8():
    from tests.emul import rm3014_emul_bind as E
    g = golden()
    assert g.dtype == np.uint32 and g.shape == (1 << 14,)
    assert np.array_equal(E.encode(np.arange(1 << 14)), g)
    assert not E.syndrome(g).any()
    w = popcount(g[1:])
    assert w.min() == 8 and int((w == 8).sum()) == 345
    tab, have = E.table()
    assert have == 4526 and tab.nbytes <= 256 << 10             # the weight <= 3 patterns have distinct syndromes; the table's size


def test_every_error_pattern_up_to_weight_3_is_corrected():
    from tests.emul import rm3014_emul_bind as E
    total = 0
    for c in four_codewords():
        for k in range(4):
            p = patterns(k)
            out, dist = E.decode(c ^ p)
            assert (out == c).all() and (dist == k).all(), (hex(int(c)), k)
            total += p.size
    assert total == 4 * 4526


def test_every_weight_4_pattern_is_refused_not_miscorrected():
    from tests.emul import rm3014_emul_bind as E
    p = patterns(4)
    assert p.size == 27405
    out, dist = E.decode(p)
    assert np.array_equal(out, p) and (dist == UNDEC).all()


def test_random_words_equal_brute_force_nearest_codeword():
    from tests.emul import rm3014_emul_bind as E
    w = random_words()
    want, want_d = np_rm3014_decode(w, golden())
    out, dist = E.decode(w)
    n_dec = int((want_d != UNDEC).sum())
    print("decodable random words:", n_dec, "of", w.size)
    assert n_dec >= 0.05 * w.size                              # expected 4526 * 2^14 / 2^30 = 6.9 %: 276 +- 16
    assert np.array_equal(out, want) and np.array_equal(dist, want_d)


def test_aach_header_symbols_exported_and_flag(pkg):
    """include/tetra_aach.h: every declared entry point is exported and bound; the flag takes the bit after ONE_STREAM and a config
    with an unknown bit is still refused before any device work."""
    import ctypes as C
    import re
    root = os.path.dirname(HERE)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "tetra_aach.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(tetra_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(pkg.lmac_binding.AACH_EXPORTS + pkg.rx_binding.RX_AACH_EXPORTS) and len(names) == 3
    L = pkg.load_library()
    for n in names:
        assert hasattr(L, n), n
    R = pkg.rx_binding
    assert R.FLAG_AACH_RM3014 == 2 and pkg.lmac_binding.JOB_RM3014 == 0x100
    assert re.search(r"TETRA_RX_FLAG_AACH_RM3014\s*=\s*2\b", open(os.path.join(root, "include", "tetra_rx.h")).read())
    assert re.search(r"#define\s+TETRA_LMAC_JOB_RM3014\s+0x100\b", src)
    R._lib()
    cfg, h = R.RxConfig(), C.c_void_p()
    assert L.tetra_rx_default_config(C.byref(cfg)) == 0
    cfg.flags = 4
    assert L.tetra_rx_create(C.byref(cfg), C.byref(h)) == -1 and not h.value        # TETRA_ERR_ARG
    n = C.c_int(5)
    assert L.tetra_rx_fetch_aach_dist(None, 0, None, 0, C.byref(n)) == -1
    assert L.tetra_lmac_rm3014_decode_device(None, -1, None, None, None) == -1 and L.tetra_lmac_rm3014_decode_device(None, 0, None, None, None) == 0


def test_gen_downlink_aach_argument_replaces_only_the_aach(synth):
    g = golden()
    aach = bits_of(g[np.arange(9) * 1111 + 5])
    a, sa = synth.gen_downlink(9, 77, cell=(300, 2000, 9))
    b, sb = synth.gen_downlink(9, 77, cell=(300, 2000, 9), aach=aach)
    assert all(np.array_equal(x[1], y[1]) for k in ("sb1", "sb2", "ndb1", "ndb2", "schf") for x, y in zip(sa[k], sb[k]))
    assert all(np.array_equal(y[1], aach[s]) for s, y in enumerate(sb["bbk"]))
    code = synth.tx_scramb_code(300, 2000, 9)
    seq = synth.tx_scramb_seq([code], 30)[0]
    a, b = a.reshape(9, 510), b.reshape(9, 510)
    for s in range(9):
        where = list(range(252, 282)) if s % 4 == 0 else list(range(230, 244)) + list(range(266, 282))
        assert np.array_equal(b[s, where] ^ seq, aach[s])
        rest = np.setdiff1d(np.arange(510), where + [12, 13, 498, 499])                     # (the phase-adjustment bits follow the content)
        assert np.array_equal(a[s, rest], b[s, rest])


# ---------------------------------------------------------------------------------------------------------------------- GPU


def _i32(torch, a, dev):
    return torch.from_numpy(np.asarray(a).astype(np.int64)).to(dev).to(torch.int32).contiguous()        # uint32 bit patterns


@pytest.mark.gpu
def test_gpu_primitive_equals_the_host_lane_code(pkg):
    import torch
    from tests.emul import rm3014_emul_bind as E
    dev = torch.device("cuda", 0)
    w, ew, ed = primitive_cases()
    w = np.concatenate([w, random_words(), np.array([0xffffffff, 0xc0000000], np.uint32)])      # (bits 31..30 are ignored)
    want, want_d = E.decode(w)
    assert np.array_equal(want[:ew.size], ew) and np.array_equal(want_d[:ed.size], ed)
    d_w = _i32(torch, w, dev)
    d_out = torch.full_like(d_w, 7)
    d_dist = torch.full((w.size,), 9, dtype=torch.uint8, device=dev)
    pkg.lmac_binding.rm3014_decode_device(d_w, w.size, d_out, d_dist)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint32), want) and np.array_equal(d_dist.cpu().numpy(), want_d)
    pkg.lmac_binding.rm3014_decode_device(d_w, w.size, d_w, d_dist)                               # in place
    torch.cuda.synchronize()
    assert np.array_equal(d_w.cpu().numpy().view(np.uint32), want)


def _seventy_blocks(synth):
    """5 channels x 14 frame slots: SYNC / NORM_1 / NORM_2 bursts from synth's builders, each AACH a golden codeword with 0..5 flipped
    bits, scrambled with its slot's own code.  -> frames [70][512], types, codes, received AACH words (descrambled), AACH type-5 rows."""
    g = golden()
    rng = np.random.default_rng(7014)
    n = 70
    types = np.array([(3, 0, 1, 0, 1, 3, 0)[r % 7] for r in range(n)], np.int32)                   # TETRA_TRAIN_SYNC / NORM_1 / NORM_2
    codes = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    words = g[rng.integers(0, 1 << 14, n)].copy()
    for r in range(n):
        for b in rng.choice(30, r % 6, replace=False):
            words[r] ^= np.uint32(1 << int(b))
    t5 = bits_of(words) ^ synth.tx_scramb_seq(codes, 30)
    frames = np.zeros((n, 512), np.uint8)
    for r in range(n):
        if types[r] == 3:
            frames[r, :510] = synth.tx_sync_burst(rng.integers(0, 2, 120), t5[r], rng.integers(0, 2, 216))
        else:
            frames[r, :510] = synth.tx_norm_burst(rng.integers(0, 2, 216), t5[r], rng.integers(0, 2, 216), int(types[r] == 1))
    return frames, types, codes, words, t5


def _expected_rows(words):
    from tests.emul import rm3014_emul_bind as E
    out, dist = E.decode(words)
    rows = np.zeros((words.size, 32), np.uint8)
    rows[:, :30] = bits_of(out)
    rows[:, 30] = dist
    return rows, (dist <= 3).astype(np.int32), dist


@pytest.mark.gpu
def test_gpu_decode_frames_rm_bbk_job_beside_the_other_kinds(pkg, synth):
    """One launch with the SCH/F, SB2 and NDB jobs and the RM BBK job over 70 frames (two workgroups of BBK rows): the BBK rows,
    crc_ok, byte 30 and labels follow tetra_aach.h's table; every other job equals a launch without the option byte for byte; and
    the BBK job without the option is the pass-through it was."""
    import torch
    from tests.emul import bsync_emul_bind
    lb = pkg.lmac_binding
    dev = torch.device("cuda", 0)
    frames, types, codes, words, _ = _seventy_blocks(synth)
    n, F = 70, 14
    want_rows, want_ok, dist = _expected_rows(words)
    assert set(np.unique(dist)) == {0, 1, 2, 3, UNDEC} and (dist == UNDEC).sum() >= 20
    d_fr = _i32(torch, bsync_emul_bind.pack_frames(frames), dev)
    d_ft = torch.from_numpy(types).to(dev)
    d_codes = _i32(torch, codes, dev)
    bitnum = torch.arange(n, dtype=torch.int32, device=dev) * 510 + 3
    t_rx = torch.arange(n, dtype=torch.int32, device=dev) + 100
    t_af = torch.arange(n, dtype=torch.int32, device=dev) + 900
    lists = {3: np.flatnonzero(types == 3), 0: np.flatnonzero(types == 0), 1: np.flatnonzero(types == 1), None: np.arange(n)}
    kinds = ((5, 0, 0, 288), (1, 2, 3, 144), (2, 1, 1, 144), (2, 2, 1, 144), (3, 0, None, 32))      # (tpsap, blk, list, row bytes)

    def launch(bbk_type):
        jobs, outs = [], []
        for tpsap, blk, li, n2 in kinds:
            rf = torch.from_numpy(lists[li].astype(np.int32)).to(dev)
            t2 = torch.full((n, n2 + 8), 5, dtype=torch.uint8, device=dev)
            ok = torch.full((n,), -3, dtype=torch.int32, device=dev)
            lab = torch.full((n, 6), -1, dtype=torch.int32, device=dev)
            outs.append((t2, ok, lab))
            jobs.append(dict(type=bbk_type if tpsap == 3 else tpsap, blk_num=blk, row_frame=rf, n_rows=None, max_rows=int(rf.numel()),
                             out_stride=n2 + 8, frame_scramb=d_codes, type2=t2, crc_ok=ok, labels=lab))
        lb.decode_frames_device(d_fr, d_ft, jobs, F, bitnum, t_rx, t_af)
        torch.cuda.synchronize()
        return [tuple(x.cpu().numpy() for x in o) for o in outs]

    plain, rm = launch(lb.TPSAP_T_BBK), launch(lb.TPSAP_T_BBK | lb.JOB_RM3014)
    for k in range(4):
        assert all(np.array_equal(a, b) for a, b in zip(plain[k], rm[k])), kinds[k]
        assert plain[k][1][:lists[kinds[k][2]].size].min() >= 0
    t2, ok, lab = rm[4]
    assert np.array_equal(t2[:, :32], want_rows) and (t2[:, 32:] == 5).all()
    assert np.array_equal(ok, want_ok)
    r = np.arange(n)
    assert np.array_equal(lab, np.stack([r // F, r % F, r * 510 + 3, r + 100, r + 900, want_ok], axis=1))
    # without the option: the 30 received bits, two zero bytes, crc_ok = 1 -- and undecodable rows with the option keep those bits
    t2p, okp, labp = plain[4]
    assert np.array_equal(t2p[:, :30], bits_of(words)) and not t2p[:, 30:32].any() and (okp == 1).all() and (labp[:, 5] == 1).all()
    bad = dist == UNDEC
    assert np.array_equal(t2[bad, :30], t2p[bad, :30])
    # the flag belongs to BBK jobs only
    with pytest.raises(pkg.TetraDemodError):
        rf = torch.zeros(1, dtype=torch.int32, device=dev)
        lb.decode_frames_device(d_fr, d_ft, [dict(type=lb.TPSAP_T_SB2 | lb.JOB_RM3014, blk_num=2, row_frame=rf, n_rows=None, max_rows=1, out_stride=144,
                                                  frame_scramb=d_codes, type2=torch.zeros(144, dtype=torch.uint8, device=dev),
                                                  crc_ok=torch.zeros(1, dtype=torch.int32, device=dev))])


@pytest.mark.gpu
def test_gpu_byte_row_entry_point_under_both_route_settings(pkg, synth):
    """The same 70 blocks as byte rows through tetra_lmac_decode_aach_rm3014_device, with tetra_lmac_debug_force_byte_route off and on
    (AACH rows have one route: the setting must not matter), next to the pass-through of tetra_lmac_decode_batch_device."""
    import torch
    lb = pkg.lmac_binding
    dev = torch.device("cuda", 0)
    _, _, codes, words, t5 = _seventy_blocks(synth)
    n = 70
    want_rows, want_ok, dist = _expected_rows(words)
    rows = np.zeros((n, 32), np.uint8)
    rows[:, :30] = t5
    d_in, d_codes = torch.from_numpy(rows).to(dev), _i32(torch, codes, dev)
    was = lb.force_byte_route(False)
    try:
        for forced in (False, True):
            lb.force_byte_route(forced)
            out = torch.full((n, 40), 5, dtype=torch.uint8, device=dev)
            ok = torch.full((n,), -3, dtype=torch.int32, device=dev)
            lb.decode_aach_rm3014_device(d_in, n, 32, d_codes, out, 40, ok)
            torch.cuda.synchronize()
            out = out.cpu().numpy()
            assert np.array_equal(out[:, :32], want_rows) and (out[:, 32:] == 5).all(), forced
            assert np.array_equal(ok.cpu().numpy(), want_ok), forced
            plain = torch.full((n, 32), 5, dtype=torch.uint8, device=dev)
            okp = torch.full((n,), -3, dtype=torch.int32, device=dev)
            lb.decode_batch_device(lb.TPSAP_T_BBK, d_in, n, 32, d_codes, plain, 32, okp)
            torch.cuda.synchronize()
            plain = plain.cpu().numpy()
            assert np.array_equal(plain[:, :30], bits_of(words)) and (plain[:, 30:] == 5).all() and (okp.cpu().numpy() == 1).all()
            assert np.array_equal(out[dist == UNDEC, :30], plain[dist == UNDEC, :30])
    finally:
        lb.force_byte_route(was)
    with pytest.raises(pkg.TetraDemodError):             # a row has to hold bytes 30 and 31
        lb.decode_aach_rm3014_device(d_in, n, 32, d_codes, torch.zeros((n, 28), dtype=torch.uint8, device=dev), 28,
                                     torch.zeros(n, dtype=torch.int32, device=dev))


# The chain's stream: 2 channels x 36 000 samples at 25 dB Es/N0, RM-coded AACHs, the error weight injected at the transmitter cycling
# 0, 1, 2, 3, 4 over the slots.  The expectations below were counted on the CPU by running this very stream through the oracle
# demodulator and the reference's own synchroniser and tp_sap_udata_ind (oracle/_ref, ReferenceRxChain: the AACH indications whose
# scrambling code is the cell's, i.e. the slots behind the first good SYNC; 3 more per channel come before it), channels summed:
#   CHAIN_EXPECT        slots per injected weight
#   CHAIN_DAMAGED       slots whose 30 descrambled bits differ from the transmitted ones: the demodulator's own bit errors (channel 0,
#                       slots 15, 16 and 28, two to three bits each) -- there the distance is not the injected weight
#   CHAIN_EXPECT_DIST   the brute-force decoder's distances over the reference-descrambled bits of those slots
# Without the three damaged slots the two histograms would be the same; weight 4 is what must come back undecodable.
CHAIN_SAMPLES, CHAIN_CHANNELS, CHAIN_SEED = 36000, 2, 9014
CHAIN_EXPECT = {0: 25, 1: 25, 2: 25, 3: 26, 4: 27}
CHAIN_DAMAGED = 3
CHAIN_EXPECT_DIST = {0: 24, 1: 24, 2: 25, 3: 28, UNDEC: 27}
CHAIN_ROWS_BEFORE_SYNC = 6


def chain_stream(synth):
    g = golden()
    n_slots = CHAIN_SAMPLES // 510 + 2
    cells = [(321 + c, 4000 + 17 * c, 11 + c) for c in range(CHAIN_CHANNELS)]
    weight = np.arange(n_slots) % 5
    tx, aachs, iq = [], [], []
    for c in range(CHAIN_CHANNELS):
        rng = np.random.default_rng(CHAIN_SEED + c)
        words = g[rng.integers(0, 1 << 14, n_slots)].copy()
        for s in range(n_slots):
            for b in rng.choice(30, int(weight[s]), replace=False):
                words[s] ^= np.uint32(1 << int(b))
        bits, _ = synth.gen_downlink(n_slots, CHAIN_SEED + 10 + c, cell=cells[c], aach=bits_of(words))
        tx.append(bits), aachs.append(words)
        iq.append(synth.gen_channel(CHAIN_SAMPLES, CHAIN_SEED + 20 + c, bits=bits, esn0_db=25.0)[0])
    return cells, weight, aachs, np.stack(iq)


def slot_of_time(t):
    """the transmitter's slot of a packed TDMA time (synth.tdma_time_of_slot inverted; mn >= 1 only behind a good SYNC PDU)"""
    tn, fn, mn = t & 0xff, (t >> 8) & 0xff, t >> 16
    return (mn - 1) * 72 + (fn - 1) * 4 + (tn - 1)


@pytest.fixture(scope="module")
def chain_runs(pkg, synth):
    """the stream through two handles, without and with the flag: fetches of every kind, the distances, the CRC-good deliveries"""
    R = pkg.rx_binding
    cells, weight, aachs, iq = chain_stream(synth)
    runs = {}
    for flags in (0, R.FLAG_AACH_RM3014):
        rx = pkg.RxChain(CHAIN_CHANNELS, CHAIN_SAMPLES, flags=flags)
        rx.process(iq)
        rx.wait()
        got = {k: rx.fetch(k) for k in range(R.N_KINDS)}
        got = {k: (b.copy(), t.copy()) for k, (b, t) in got.items()}
        if flags:
            dist = rx.fetch_aach_dist().copy()
            assert rx.rows_device(R.KIND_BBK)[1] == 32
        else:
            dist = None
            with pytest.raises(pkg.TetraDemodError):
                rx.fetch_aach_dist()
        dl = rx.deliver(kinds=1 << R.KIND_BBK, crc_good_only=True).wait()[R.KIND_BBK]
        runs[flags] = dict(got=got, dist=dist, good=(dl[0].copy(), dl[1].copy()))
        rx.close()
    return cells, weight, aachs, runs


@pytest.mark.gpu
def test_gpu_chain_with_the_flag_corrects_and_flags_the_aach(pkg, synth, chain_runs):
    R = pkg.rx_binding
    cells, weight, aachs, runs = chain_runs
    plain, rm = runs[0], runs[R.FLAG_AACH_RM3014]
    for k in range(R.N_KINDS):
        if k != R.KIND_BBK:
            assert np.array_equal(plain["got"][k][0], rm["got"][k][0]) and np.array_equal(plain["got"][k][1], rm["got"][k][1]), k
    (pb, pt), (rb, rt) = plain["got"][R.KIND_BBK], rm["got"][R.KIND_BBK]
    assert len(pb) == len(rb) > 120 and (pb["crc_ok"] == 1).all()
    want, want_d = np_rm3014_decode(words_of(pt), golden())              # every row, incl. those before the first good SYNC (code 0)
    assert np.array_equal(rt, bits_of(want)) and np.array_equal(rm["dist"], want_d)
    assert np.array_equal(rb["crc_ok"], (want_d <= 3).astype(np.int32))
    for f in ("channel", "frame_slot", "bitnum", "tdma_time_rx", "tdma_time"):
        assert np.array_equal(pb[f], rb[f]), f
    # coverage: behind the first good SYNC a row's time names the transmitter's slot, so its injected weight is known
    post = (rb["tdma_time"] >> 16) != 0
    assert (~post).sum() == CHAIN_ROWS_BEFORE_SYNC
    hist, damaged = {w: 0 for w in range(5)}, 0
    for j in np.flatnonzero(post):
        c, s = int(rb["channel"][j]), slot_of_time(int(rb["tdma_time"][j]))
        w = int(weight[s])
        hist[w] += 1
        sent = aachs[c][s]
        if not np.array_equal(pt[j], bits_of([sent])[0]):               # the demodulator's own bit errors on top: only the brute force speaks
            damaged += 1
        elif w <= 3:
            assert rm["dist"][j] == w and rb["crc_ok"][j] == 1 and popcount(words_of(rt[j:j + 1]) ^ sent)[0] == w
        else:
            assert rm["dist"][j] == UNDEC and rb["crc_ok"][j] == 0 and np.array_equal(rt[j], pt[j])
    hist_d = {int(d): int((rm["dist"][post] == d).sum()) for d in (0, 1, 2, 3, UNDEC)}
    print("AACH rows behind the first good SYNC per injected weight:", hist, "damaged by the channel:", damaged, "per distance:", hist_d)
    assert hist == CHAIN_EXPECT and damaged == CHAIN_DAMAGED and hist_d == CHAIN_EXPECT_DIST


@pytest.mark.gpu
def test_gpu_crc_good_delivery_keeps_exactly_the_decodable_aach_rows(pkg, chain_runs):
    R = pkg.rx_binding
    _, _, _, runs = chain_runs
    plain, rm = runs[0], runs[R.FLAG_AACH_RM3014]
    rb, rt = rm["got"][R.KIND_BBK]
    keep = rb["crc_ok"] != 0
    assert 0 < keep.sum() < len(rb)
    gb, gt = rm["good"]
    assert np.array_equal(gb, rb[keep]) and np.array_equal(gt[:, :30], rt[keep])
    pb, pt = plain["got"][R.KIND_BBK]
    gb, gt = plain["good"]
    assert np.array_equal(gb, pb) and np.array_equal(gt[:, :30], pt)         # without the flag: every AACH row, as before


@pytest.mark.gpu
def test_gpu_wideband_handle_accepts_the_flag(pkg):
    R = pkg.rx_binding
    wb = pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=1 << 16, flags=R.FLAG_AACH_RM3014)
    assert wb.rx.fetch_aach_dist().size == 0                                 # the chain inside carries the option; no call yet
    wb.close()
    with pytest.raises(pkg.TetraDemodError):
        pkg.WidebandRx([1, 7, 20], n_channels=32, decimation=16, max_in=1 << 16, flags=4)
