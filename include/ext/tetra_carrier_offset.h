/*
 * tetra_carrier_offset.h -- C ABI of the wideband receiver's per-carrier mixer: every carrier slot may lie off its bin's centre by
 * an offset of its own.
 *
 * The channeliser's shift (tetra_shift.h) moves ALL bins by one common offset: a raster offset, an SDR tuning offset.  It does not
 * cover a band that mixes rasters in one capture, carriers of several networks whose own frequency error is beyond what the
 * demodulator's FLL pulls in, or one carrier that sits a few kHz off its bin.  The reference plugin meets these with one VFO per
 * instance (src/main.cpp:75).  Here the selecting resampler, which touches exactly the carriers' columns, rotates each column as it
 * loads it:
 *
 *     y[m][j] = sum_{t<T} h[r_m + I t] . x[q_m - t][bins[j]] . exp(-j 2 pi ((inc_j (q_m - t)) mod 2^32) / 2^32)
 *
 * = the resampler of tetra_chan.h run on slot j's channeliser column pre-multiplied by exp(-j 2 pi inc_j n / 2^32), n = the absolute
 * index of the channeliser frame since create / tetra_wbrx_reset.  inc_j / 2^32 is in cycles per channeliser OUTPUT frame: a carrier
 * f Hz above its bin's centre needs inc = f . D / Fs . 2^32 (D = the channeliser's decimation, Fs = the capture's rate).
 *
 * The phase is formed in integer arithmetic, so the result is exact at any stream position and for any cut of the capture; no
 * floating-point phase is carried from row to row or call to call.  Results are held to the float32 tolerance of the shifted bank
 * against the double-precision definition (2e-5 of the output's maximum; measured 3.5e-7 at worst: DESIGN.md 8.12).
 *
 * Reach.  The bank is 2 x oversampled (bins Fs / M apart, frames at 2 Fs / M): an off-centre carrier must still fit inside the bin
 * prototype's passband, and what the prototype leaves of the neighbouring spectrum must stay outside the carrier's own +-12.5 kHz after
 * the mixer.  The offset a bin can serve therefore depends on chan_cutoff_rel and taps_per_channel.  The middle between the two edges
 * is the bin spacing whatever the offset, so the documented choice is chan_cutoff_rel = 2.0; with it, on a band without carriers on
 * neighbouring bins, every block decodes up to |offset| = 3.125 kHz at taps_per_channel 8 and up to 12.5 kHz (the whole range measured,
 * in steps of 1.5625 kHz) at taps_per_channel 16.  An offset of half a bin common to all carriers stays the shift's job.
 *
 * These entry points extend the handle of tetra_wbrx.h.  They live in a header of their own because that header's entry-point list is
 * pinned by count, as are the config structs and TETRA_DEMOD_ABI_VERSION: none of that changes.
 */
#ifndef TETRA_CARRIER_OFFSET_H
#define TETRA_CARRIER_OFFSET_H

#include <stdint.h>

#include "../tetra_wbrx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* inc [n_bins]: slot j's offset, 2^-32 cycles per channeliser frame.  All zero is the default: then the kernels launched are the ones
 * a handle without this header launches, and every output bit is the same.
 *
 * Callable between process calls.  The list is copied before the call returns; the upload is enqueued on hip_stream behind the last
 * process call's work and ahead of the next call's resampler, whatever stream that call is given (the ordering rules of
 * tetra_wbrx_retune).  The outputs of a call depend on the offsets in force at that call only: from the next call on the handle gives
 * what a handle that had these offsets from the start would give -- the delay line and the retune ring keep un-rotated frames, and the
 * phase reference n is not restarted.  On the carrier this is one phase step, which the differential demodulator does not see.
 * A list equal to the one in force enqueues nothing.
 *
 * tetra_wbrx_retune: a slot keeps its offset when its bin changes; to change both, call this in the same gap.
 * tetra_wbrx_reset keeps the offsets and restarts n.  tetra_wbrx_frames_device returns the mixed frames.  tetra_wbrx_bin_power is
 * taken in front of the mixer and does not change.  The channeliser's shift and the offsets compose (shift first).
 * A handle created with bins 0 .. M - 1 in order resamples in place; its first non-zero offset moves it to the selecting resampler
 * for good, as its first retune does.
 *
 * TETRA_ERR_ARG: NULL handle or list.  TETRA_ERR_NO_DEVICE: no device (whatever the arguments).  TETRA_ERR_HIP / _NO_DEVICE leave the
 * previous offsets in force. */
int tetra_wbrx_set_carrier_offsets(tetra_wbrx_t* h, const uint32_t* inc, void* hip_stream);
/* inc [n_bins]: the offsets in force. */
int tetra_wbrx_get_carrier_offsets(tetra_wbrx_t* h, uint32_t* inc);
/* round(offset_hz . decimation / sample_rate_hz . 2^32) mod 2^32; negative offsets wrap (-f gives 2^32 - inc(f)).  0 for a sample
 * rate <= 0, a decimation < 1 or an offset that is not finite (the rules of tetra_chan_shift_from_hz). */
uint32_t tetra_wbrx_carrier_offset_from_hz(double offset_hz, double sample_rate_hz, int decimation);

#ifdef __cplusplus
}
#endif
#endif
