"""The receive chain's soft AACH option (TETRA_RX_FLAG_SOFT | TETRA_RX_FLAG_AACH_SOFT) restated on the host for
tests/test_aach_soft_gpu.py, beside tests/soft_pipeline.py and in its way: oracle symbols -> quantiser (numpy binary32) -> per frame the
AACH's 30 ring positions descrambled by sign under the reference's clock and scrambling codes -> the numpy definition
(tests/aach_soft_definition.py).  The coded kinds go through the reference's soft decoder as in soft_pipeline (an SB1 with a good CRC sets
the code the burst's AACH is descrambled with).  Nothing of the product's code runs here.  Needs oracle/_ref."""
import numpy as np

from tests import aach_soft_definition as A
from tests import chain_host as ch
from tests import soft_pipeline as sp

# The stream of tests/golden/aach_soft_golden.npz: the size of tests/chain_host.py's operating point, RM-coded AACHs, and a level chosen
# on the CPU (see test_aach_soft_gpu.py's constants) at which the hard rule loses rows that maximum likelihood keeps.
CHANNELS, SLOTS, SAMPLES, SEED = 5, 71, 36000, 9401
ESN0_DB = 9.5


def sent_info():
    """int [CHANNELS][SLOTS]: the information bits of every slot's AACH"""
    return np.stack([np.random.default_rng(SEED + 50 + c).integers(0, 16384, SLOTS) for c in range(CHANNELS)])


def stream_iq(synth):
    return ch.downlink_batch(synth, CHANNELS, SLOTS, SAMPLES, SEED, ESN0_DB, aach=A.code_bits()[sent_info()])[2]


def slot_of_time(t):
    """the transmitter's slot of a packed TDMA time (synth.tdma_time_of_slot inverted; mn >= 1 only behind a good SYNC PDU)"""
    tn, fn, mn = t & 0xff, (t >> 8) & 0xff, t >> 16
    return (mn - 1) * 72 + (fn - 1) * 4 + (tn - 1)


def slots_of(label, n_slots=SLOTS):
    """The transmitter's slot of every row, from its frame's bit number: frames lie 510 bits apart, and where in the demodulator's bit
    stream slot 0 starts is what most of the channel's good clock readings agree on (a receiver clock that free-runs over a lost SYNC
    PDU may name another slot; the bit number does not)."""
    out = np.zeros(len(label), np.int64)
    for c in np.unique(label[:, 0]):
        rows = np.flatnonzero(label[:, 0] == c)
        timed = rows[(label[rows, 3] >> 16) != 0]
        start = label[timed, 1] - 510 * np.array([slot_of_time(int(t)) for t in label[timed, 3]])
        vals, counts = np.unique(start, return_counts=True)
        out[rows] = np.rint((label[rows, 1] - vals[counts.argmax()]) / 510.0).astype(np.int64) if len(vals) else 0
    return np.clip(out, 0, n_slots - 1)


def channel_aach(ref, oracle, bits, soft, channel):
    """One channel's stream -> per frame, in frame order: label (channel, bitnum, time on entry, time), the AACH's 30 hard bits
    descrambled, its 30 soft values descrambled by sign.  tests/chain_host.walk under the reference's clock and scrambling codes, the
    SB1 through the reference's soft decoder: a good CRC sets clock and code for the burst's AACH."""
    frames, types, bitnums = oracle.BurstSyncOracle().feed(bits, chunk=1)
    labels, hard, values = [], [], []
    sb1 = lambda f: sp.ref_soft_decode(ref, 0, ch.cut(soft, int(bitnums[f]), ch.BLOCK[(ch.TRAIN_SYNC, ch.KIND_SB1)].pieces), 0)
    for f, (code, t_rx, t_af, _) in enumerate(ch.walk(types, ch.ref_clock(ref), sb1, ref.scramb_get_init)):
        if int(types[f]) not in ch.BURST_KINDS:
            continue
        pieces = ch.BLOCK[(int(types[f]), ch.KIND_BBK)].pieces
        seq = sp.scramb_seq(ref, code, 30)
        labels.append((channel, int(bitnums[f]), t_rx, t_af))
        hard.append(ch.cut(frames[f], 0, pieces) ^ seq)
        values.append(A.descramble(ch.cut(soft, int(bitnums[f]), pieces), seq))
    return labels, hard, values


def stream_aach(ref, oracle, iq):
    """iq complex64 [C][N] -> dict: label int64 [n][4], hard uint8 [n][30], soft int8 [n][30]; all channels, channel-major"""
    labels, hard, values = [], [], []
    for c, (bits, soft) in enumerate(zip(*sp.oracle_streams(oracle, iq))):
        l, h, v = channel_aach(ref, oracle, bits, soft, c)
        labels += l
        hard += h
        values += v
    return dict(label=np.array(labels, np.int64).reshape(-1, 4), hard=np.array(hard, np.uint8).reshape(-1, 30), soft=np.array(values, np.int8).reshape(-1, 30))


def hard_rm(hard_bits):
    """The radius-3 rule of tetra_aach.h by brute force over the recorded codewords: bits [n][30] -> (info or -1 where no codeword lies
    within 3 bit errors, the distance to the nearest codeword)."""
    d = (np.asarray(hard_bits)[:, None, :] != A.code_bits()[None, :, :]).sum(axis=2)
    best = d.argmin(axis=1)
    dist = d[np.arange(len(d)), best]
    return np.where(dist <= 3, best, -1), dist


def scores(g):
    """Of the fixture's rows behind the first good SYNC PDU (the code they are descrambled with is then the cell's; their slot comes from
    slots_of): per decoder (pass-through, hard RM,
    ML at min_margin 1) the rows equal to the sent codeword, accepted but wrong, and refused -> dict name -> (right, wrong, refused), and
    the rows' count, ML's margins of its right and of its wrong rows."""
    lab = g["label"]
    post = (lab[:, 3] >> 16) != 0
    sent = sent_info()[lab[post, 0], slots_of(lab)[post]]
    hard, soft = g["hard"][post], g["soft"][post]
    plain_right = (hard == A.code_bits()[sent]).all(axis=1)
    rm, _ = hard_rm(hard)
    info, margin, _ = A.decode(soft)
    ml_acc = margin >= 1
    out = {"pass": (int(plain_right.sum()), int((~plain_right).sum()), 0),
           "rm": (int((rm == sent).sum()), int(((rm != sent) & (rm >= 0)).sum()), int((rm < 0).sum())),
           "ml": (int(((info == sent) & ml_acc).sum()), int(((info != sent) & ml_acc).sum()), int((~ml_acc).sum()))}
    return out, int(post.sum()), margin[info == sent], margin[info != sent]
