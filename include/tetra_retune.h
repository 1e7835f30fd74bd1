/*
 * tetra_retune.h -- C ABI of retuning while the stream runs: restart single channels of the receive chain (tetra_rx.h), and move the
 * wideband receiver's carrier slots (tetra_wbrx.h) to other bins, without a host synchronisation and without touching the rest.
 *
 * A trunked network announces traffic carriers on its control channel; a monitor must start receiving one within a frame or two
 * and drop it when the call ends.  Destroying and re-creating the handle for that throws away the loop lock, burst sync, cell state
 * and TDMA clock of every other carrier and restarts the channeliser's and the resampler's delay lines.  Here a wideband handle
 * created with n_bins = S is a bank of S receiver slots: slot j receives bin bins[j], and a retune hands in a new list of S bins.
 *
 * These entry points extend the handles of tetra_rx.h and tetra_wbrx.h.  They live in a header of their own because the entry-point
 * lists of those headers are pinned by count (tests/test_abi.py, tests/test_wbrx.py), as are their config structs and
 * TETRA_DEMOD_ABI_VERSION: none of that changes.  On a machine without a HIP device every entry point returns TETRA_ERR_NO_DEVICE.
 */
#ifndef TETRA_RETUNE_H
#define TETRA_RETUNE_H

#include <stdint.h>

#include "tetra_rx.h"
#include "tetra_wbrx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Leaves the n listed channels as tetra_rx_reset leaves ALL channels -- demodulator loops as tetra_demod_reset(h, channel) under the
 * handle's flags (TETRA_FLAG_REFERENCE_QUIRKS: the reference's reset to the letter), synchroniser UNLOCKED and empty, cell state and
 * TDMA clock zero, bit numbering from 0 -- and every other channel, the call counter and the results of earlier calls as they are.
 *
 * Takes effect between the last enqueued process call and the next one: from the next call on, a listed channel's output is that of
 * a fresh handle's channel fed the same samples.  Enqueued, not waited for: the demodulator's state is reset on hip_stream behind
 * the demodulator of the last call, the synchroniser's and the cell state on the stream the chain's tail runs on, behind that
 * call's tail; the next tetra_rx_process_device is ordered behind both on whatever stream it is given.  tetra_rx_wait, _fetch,
 * _get_cell and _get_sync_state see the reset once it has run.
 *
 * channels: a host list, copied before the call returns.  n = 0 does nothing.  TETRA_ERR_ARG: a NULL list with n > 0, n < 0 or
 * n > the chain's channels, an index outside [0, n_channels), a duplicate index; nothing is enqueued then.  The list travels through
 * a ring of four page-locked blocks (allocated by the first call): a fifth call blocks only while the first's kernels have not run.
 *
 * Not for a chain that a wideband handle owns (tetra_wbrx_rx): like tetra_rx_process, _reset and _destroy it is the wideband
 * handle's to call -- tetra_wbrx_retune does, for the slots it moves, together with the slot's resampler column.  This entry point
 * refuses such a chain: TETRA_ERR_UNSUPPORTED, nothing enqueued. */
int tetra_rx_reset_channels_device(tetra_rx_t* h, const int32_t* channels, int n, void* hip_stream);

/* bins [n_bins]: the new bin of every slot.  Takes effect between the last enqueued tetra_wbrx_process* call and the next one.
 *
 * A slot whose bin stays is not touched in any stage: its resampled IQ, bits, blocks, labels, bit numbers, cell, sync and demodulator
 * state are those of a handle that was never retuned, bit for bit, call for call.  Every other slot -- also one whose new bin was
 * another slot's before: state is not permuted -- starts afresh on its new bin:
 *   - its resampled IQ from the next call on is column new_bin of tetra_resamp run on all M bins of the same capture, bit for bit
 *     from the first frame and for any cut of the capture.  (The resampler's output position is common to all channels; the slot's
 *     T - 1 delay-line frames are rebuilt from the channeliser's output of the new bin, of which the handle keeps the newest T - 1
 *     frames of all M bins -- 8 (T - 1) M bytes, 96 KB at the defaults, brought up to date by one small copy kernel per call.)
 *   - its chain state is what tetra_rx_reset_channels_device leaves, so its blocks from the retune on are those of a fresh tetra_rx
 *     channel fed the slot's frames from that point.
 * The results of the calls before the retune stay fetchable under the which = 0 / 1 rules, with the slots' old meaning.
 * tetra_wbrx_bins returns the new list as soon as this returns.  The frequency shift (tetra_shift.h) is not touched.  A list equal
 * to the current one changes nothing and enqueues nothing.  A handle created with bins 0 .. M - 1 in order resamples all rows in
 * place; its first retune that changes a slot moves it to the selecting resampler for good, which gives the same floats.
 *
 * Enqueued, not waited for, ordered as tetra_rx_reset_channels_device orders its part; the bin list and the delay-line columns are
 * rewritten on hip_stream behind the last call's resampler.  Pass the stream the process calls use, or none of this needs care:
 * the next process call is ordered behind the retune on any stream.
 *
 * TETRA_ERR_ARG: bins NULL, a bin outside [0, M), a duplicate bin; nothing changes then, the device's bin list included.
 * TETRA_ERR_HIP: if enqueueing failed before the bin list moved, nothing has changed; otherwise the new list is in force
 * (tetra_wbrx_bins tells which) and the moved slots' chain state is undefined until tetra_wbrx_reset. */
int tetra_wbrx_retune(tetra_wbrx_t* h, const int32_t* bins, void* hip_stream);

/* Bookkeeping: retunes that were accepted (those that changed nothing included) and the slots they moved, since create.  Either
 * pointer may be NULL.  tetra_wbrx_reset keeps the counts (and the bin list). */
int tetra_wbrx_retune_count(tetra_wbrx_t* h, int64_t* retunes, int64_t* slots_changed);

#ifdef __cplusplus
}
#endif
#endif
