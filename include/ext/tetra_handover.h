/*
 * tetra_handover.h -- C ABI of the retune with a donor: a restarted channel inherits frame timing, cell and TDMA clock from another.
 *
 * A channel that tetra_rx_reset_channels_device / tetra_wbrx_retune (tetra_retune.h) restarts is UNLOCKED with a zero cell state: it
 * looks for the SYNC training sequence only and has no scrambling code and no TDMA clock until a SYNC PDU with a good CRC has been
 * decoded.  A carrier sends one SYNC burst per multiframe (72 slots, 1.02 s), so a slot moved onto a traffic carrier delivers nothing
 * for up to a second -- the start of the call it was moved for.  The carriers of one base station are frame-synchronous and share MCC,
 * MNC and colour code, and a terminal that follows a channel allocation carries its slot timing, scrambling code and TDMA clock over.
 * The entry points here do that on the device, with no host synchronisation: the restarted channel (the heir) takes them from another
 * channel of the same handle (the donor), which sees the same sample timeline -- the channels of a chain get the same n_samples per
 * call, the slots of a wideband handle the same resampled frames.
 *
 * This DEPARTS FROM THE REFERENCE, like ext/tetra_sync_tol.h, and is opt-in: a handle that never hands over allocates, launches and
 * computes what it always did.  The rule, in integer arithmetic on bit positions only:
 *
 * Planting, on the stream the chain's tail runs on, behind the last call's tail and behind the reset of the heir:
 *   1. read the donor's synchroniser state and cell;
 *   2. a donor that is not LOCKED, or whose scramb_init is 0: the heir stays as the plain reset left it, status REFUSED;
 *   3. else F = the donor's bitbuf_start_bitnum (the start of its next unconsumed frame), B = F + bits_in_buf (all the bits it has
 *      received), T = its PHY time;
 *   4. the heir's bit numbering starts at 0 here: expect = (F - B) + 510 m, m the smallest integer with expect - W >= 0;
 *   5. the heir's cell = the donor's: scramb_init, colour code, MCC, MNC, tcd_tn / fn / mn;
 *   6. its PHY time = T advanced by m slots, in tetra_tdma_time_add_tn steps (wrap thresholds of the reference's tetra_tdma.c:28-78);
 *   7. its synchroniser enters the state ASSIST (TETRA_BSYNC_STATE_ASSIST, beside the reference's three) with expect, W and
 *      slots_left = max_slots; status PENDING.
 * ASSIST, in the synchroniser:
 *   nothing happens until the channel has received expect + W + 510 bits.  Then the candidate frame starts s = expect + d are tried in
 *   the order d = 0, +1, -1, +2, -2, ..., +W, -W; a candidate matches when the 510 bits from s hold the sync training sequence exactly
 *   at offset 214, or normal training sequence 1 or 2 exactly at offset 244.
 *   First match: everything before s is dropped, bitbuf_start_bitnum = s, next_frame_start_bitnum = s + 510, the state is LOCKED and the
 *     walk goes on under the handle's lock rule (the reference's or the tolerant one), so the matched frame is consumed as any LOCKED
 *     frame is; status LOCKED, offset = d, and 1 + k goes to the channel's result word, k = the slot periods ASSIST advanced.
 *   No match: expect += 510, the bits before expect - W are dropped, slots_left -= 1, slots_waited += 1; at slots_left = 0 the state is
 *     UNLOCKED on what is buffered, with the reference's rule from there; status EXPIRED, result word -1.
 *   The outcome does not depend on how the stream is cut into calls.
 * Apply, one small kernel in the tail between the synchroniser and the SYNC tracker (launched only on a handle that has ever handed over):
 *   result 1 + k: the channel's PHY time advances by k slots, so that the tracker's own per-frame increment gives the locked frame the
 *     time T + m + k + 1;  result -1: the channel's cell state is zeroed -- a failed hand-over leaves what a plain restart leaves.
 *
 * A donor on another cell costs nothing beyond the plain restart: the heir locks, its blocks fail their CRC until the carrier's own
 * SYNC PDU arrives and sets code and clock, as it does for every receiver.
 *
 * The default window rests on a measurement (profiles/measure_handover_window.py): a freshly reset demodulator's bit
 * stream against a running one's on the same samples is displaced by 0 or 2 bits (one symbol), at Es/N0 11, 20 and 25 dB alike; the
 * default is twice the largest magnitude seen, rounded up to a multiple of 8.  With W = 8 an exact match of a normal training sequence
 * on random payload appears somewhere in the window with probability 17 * 2 * 2^-22 = 8 * 10^-6 per slot period.
 *
 * tetra_bsync_state_t is unchanged; the hand-over's fields live beside it.  Same conventions as tetra_rx.h: extern "C", int status,
 * GPU only; on a machine without a HIP device every entry point returns TETRA_ERR_NO_DEVICE.
 */
#ifndef TETRA_HANDOVER_H
#define TETRA_HANDOVER_H

#include <stdint.h>

#include "../tetra_retune.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tetra_handover_params {
    int32_t window;    /* W: 0 .. 127 bits either side of the expected frame start */
    int32_t max_slots; /* 1 .. 255 slot periods before giving up */
} tetra_handover_params_t;

#define TETRA_HANDOVER_DEFAULT_WINDOW 8
#define TETRA_HANDOVER_DEFAULT_MAX_SLOTS 72 /* one multiframe: after that the SYNC burst the plain rule waits for has passed anyway */

/* tetra_bsync_state_t.state of a channel that waits for its inherited frame start */
#define TETRA_BSYNC_STATE_ASSIST 3

enum {
    TETRA_HANDOVER_NONE = 0,    /* never handed over, or restarted plainly since */
    TETRA_HANDOVER_PENDING = 1, /* in ASSIST */
    TETRA_HANDOVER_LOCKED = 2,  /* found its frame start in the window */
    TETRA_HANDOVER_EXPIRED = 3, /* max_slots slot periods without a match: UNLOCKED, cell state zero */
    TETRA_HANDOVER_REFUSED = 4  /* the donor was not LOCKED or had no scrambling code: a plain restart */
};

typedef struct tetra_handover_status {
    int32_t state;        /* TETRA_HANDOVER_* */
    int32_t slots_waited; /* slot periods ASSIST advanced without a match */
    int32_t offset;       /* found frame start - expected frame start, in bits (LOCKED only) */
} tetra_handover_status_t;

/*
 * Everything tetra_rx_reset_channels_device does for the n listed channels -- same ordering and streams, same list ring (its blocks
 * grow once to hold the donors), same refusal of a chain that a wideband handle owns (TETRA_ERR_UNSUPPORTED) --, then the planting for
 * every entry with donors[i] >= 0; donors[i] == -1 makes entry i a plain restart.  p == NULL: the defaults above.
 * TETRA_ERR_ARG: whatever the plain call refuses, a NULL donor list with n > 0, a donor outside [0, n_channels) other than -1, a donor
 * that is itself in `channels`, a window or max_slots out of range; nothing is enqueued then.  The first hand-over of a handle allocates
 * the per-channel fields (32 bytes per channel) and waits for the device once; from then on the handle's tails run the ASSIST-capable
 * synchroniser kernel and the apply kernel.
 */
int tetra_rx_handover_channels_device(tetra_rx_t* h, const int32_t* channels, const int32_t* donors, int n, const tetra_handover_params_t* p,
                                      void* hip_stream);

/*
 * tetra_wbrx_retune plus the hand-over for the slots that move and have a donor.  donors [n_bins]: per slot the donor slot, or -1 for a
 * plain restart; the entry of a slot that does not move is ignored.  A donor must be a slot whose bin stays.  donors == NULL is
 * tetra_wbrx_retune.  A list equal to the current one still changes nothing.  TETRA_ERR_ARG: whatever tetra_wbrx_retune refuses, a
 * moving slot's donor outside [0, n_bins) other than -1 or itself moving, parameters out of range; nothing changes then.
 */
int tetra_wbrx_retune_from(tetra_wbrx_t* h, const int32_t* bins, const int32_t* donors, const tetra_handover_params_t* p, void* hip_stream);

/* Channels first .. first + count - 1; waits for the latest call's tail, like tetra_rx_get_cell (valid on tetra_wbrx_rx(h) too).  A handle
 * that never handed over answers TETRA_HANDOVER_NONE for every channel. */
int tetra_rx_get_handover(tetra_rx_t* h, int first, int count, tetra_handover_status_t* out);

#ifdef __cplusplus
}
#endif
#endif
