/*
 * tetra_sync_tol.h -- C ABI of the burst synchroniser's tolerant training-sequence match in lock.
 *
 * The burst synchroniser (tetra_burst_sync.h) is bit-exact with the reference's tetra_burst_sync_in.  That holds for the default and is
 * not touched by anything declared here.  In LOCKED the reference accepts a burst only where tetra_find_train_seq finds a training
 * sequence without a single bit error (22 of 22 bits of a normal, 38 of 38 of the sync sequence), and a frame without any exact match
 * sends the receiver back to UNLOCKED, from where it needs 1020 buffered bits and an exact sync sequence again.  At low Es/N0 that, not
 * the decoder, decides how many bursts are delivered.
 *
 * The entry points here switch a handle to a rule that DEPARTS FROM THE REFERENCE -- an opt-in flywheel for a receiver that already
 * knows the frame timing.  Per channel, in integer arithmetic:
 *
 *   UNLOCKED and KNOW_FSTART: the reference's rules to the letter (the 1020-bit wait, the first exact sync match with its misaligned
 *   look-ahead zone, + 296, the fall-through into LOCKED).
 *   LOCKED: a frame is consumed whenever at least 510 bits are buffered, as ever.  For f = the first 510 buffered bits
 *       dS = Hamming distance of f[214 .. 251] to the sync sequence y (38 bits)
 *       d1 = distance of f[244 .. 265] to the normal sequence n,  d2 = distance of f[244 .. 265] to p
 *     candidates: SYNC if dS <= tol_sync, NORM_1 if d1 <= tol_norm, NORM_2 if d2 <= tol_norm.  The candidate with the smallest distance
 *     is reported; ties go to SYNC, then NORM_1, then NORM_2.  A reported frame sets the channel's miss counter to 0.  No candidate:
 *     frame_type = -1 and the miss counter goes up by one; when it reaches max_miss the receiver goes to UNLOCKED and the counter
 *     returns to 0.  Nothing else of the buffer is searched: a sequence at another offset neither drops the frame nor unlocks.
 *
 * Buffer handling, bit numbers and the frame record are those of tetra_burst_sync.h; the result depends on bit positions only, not on
 * how the stream is cut into calls.  tetra_bsync_state_t is unchanged; the miss counters live beside it.
 * With {0, 0, 1} a clean downlink gives the reference's frames, except where payload imitates a training sequence ahead of the expected
 * offset (the reference drops or unlocks on such a frame; this rule does not look there).
 * Same conventions as tetra_burst_sync.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_SYNC_TOL_H
#define TETRA_SYNC_TOL_H

#include <stdint.h>

#include "../tetra_burst_sync.h"
#include "../tetra_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tetra_bsync_tolerance {
    int32_t tol_norm; /* 0 .. 4: bit errors accepted in a normal training sequence (two normal sequences differ in 11 bits) */
    int32_t tol_sync; /* 0 .. 6: bit errors accepted in the sync training sequence */
    int32_t max_miss; /* 1 .. 255: consecutive frames without a candidate before the receiver falls back to UNLOCKED */
} tetra_bsync_tolerance_t;

/* What TETRA_RX_FLAG_SYNC_TOLERANT creates a chain with. */
#define TETRA_SYNC_TOL_DEFAULT_NORM 3
#define TETRA_SYNC_TOL_DEFAULT_SYNC 5
#define TETRA_SYNC_TOL_DEFAULT_MISS 16

/*
 * Switches the handle's channels to the tolerant rule with *tol, or -- tol == NULL -- back to the reference's rule.  Values out of range:
 * TETRA_ERR_ARG, and nothing changes.  Waits for the device, zeroes every channel's miss counter, and takes effect with the next process
 * call.  State, bit buffer and bit numbering of the channels carry on.  The counters (4 bytes per channel) are allocated by the first
 * switch to the tolerant rule: a handle that never leaves the reference's rule allocates and launches what it always did.
 */
int tetra_bsync_set_tolerance(tetra_bsync_t* h, const tetra_bsync_tolerance_t* tol);
/* Miss counters of channels first .. first + count - 1 (0 under the reference's rule); waits for the device like tetra_bsync_get_state. */
int tetra_bsync_get_misses(tetra_bsync_t* h, int first, int count, int32_t* out);

/*
 * The receive chain (tetra_rx.h): TETRA_RX_FLAG_SYNC_TOLERANT in tetra_rx_config_t.flags creates the chain with the defaults above;
 * through cfg.rx also for tetra_wbrx_create.  tetra_rx_set_sync_tolerance changes the rule of a chain created with or without the flag
 * (NULL: the reference's rule); callable between process calls, it waits for the tail in flight; valid on tetra_wbrx_rx(h) too.
 * tetra_rx_reset zeroes the miss counters; tetra_rx_reset_channels_device (tetra_retune.h), and with it tetra_wbrx_retune, zero those of
 * the listed channels in stream order.
 */
int tetra_rx_set_sync_tolerance(tetra_rx_t* h, const tetra_bsync_tolerance_t* tol);
/* Channels first .. first + count - 1; waits for the latest call's tail, like tetra_rx_get_sync_state.
 * Statuses: both chain entries answer like the chain's other getters (TETRA_ERR_ARG for a NULL handle or a range outside the channels,
 * TETRA_ERR_NO_DEVICE where the handle's device cannot be selected, TETRA_ERR_HIP for a failing runtime call); the two tetra_bsync_*
 * entries like tetra_bsync_get_state (TETRA_ERR_ARG, TETRA_ERR_HIP; TETRA_ERR_NOMEM where the counters cannot be allocated). */
int tetra_rx_get_sync_misses(tetra_rx_t* h, int first, int count, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif
