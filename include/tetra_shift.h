/*
 * tetra_shift.h -- C ABI of the frequency-shifted channeliser: receive carriers that lie OFF the bins' centres.
 *
 * TETRA carriers lie on a 25 kHz raster, but the raster has a band-dependent offset (12.5 kHz or 6.25 kHz against round
 * frequencies) and an SDR is tuned where its LO and its DC spike allow: all carriers of a capture are then off the centres k Fs / M
 * of the channeliser's bins (tetra_chan.h) by ONE common fraction of a bin.  The reference plugin meets this with one mixer per
 * carrier (SDR++'s VFO, src/main.cpp:75).  Because the offset is common, the bank needs neither a per-carrier mixer nor a
 * per-sample oscillator: the shift folds into it exactly,
 *
 *     x'[n] = x[n] exp(-j 2 pi delta n)                      delta = shift in cycles per input sample, n = absolute sample index
 *     out'[m][k] = exp(-j 2 pi delta n_m) . sum_l hc[l] x[n_m - l] exp(-j 2 pi k (n_m - l) / M),    hc[l] = h[l] exp(+j 2 pi delta l)
 *
 * = the bank of tetra_chan.h with a complex (modulated) prototype and one phasor per output frame, the same for all bins.  The
 * capture is still read once, in place, in its native format (complex64 / cs16 / cs8).
 *
 * These entry points extend the handles of tetra_chan.h and tetra_wbrx.h.  They live in a header of their own because the entry-point
 * lists of those two headers are pinned by count (tests/test_abi.py: 11 tetra_chan_*, tests/test_wbrx.py: 14 tetra_wbrx_*), as are
 * their config structs and TETRA_DEMOD_ABI_VERSION: none of that changes.
 */
#ifndef TETRA_SHIFT_H
#define TETRA_SHIFT_H

#include <stdint.h>

#include "tetra_chan.h"
#include "tetra_wbrx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* delta = inc / 2^32 cycles per input sample; 0 = off (the default: the un-shifted kernels run, instruction for instruction).
 *
 * With shift inc the handle's output equals the un-shifted bank run on x[n] exp(-j 2 pi inc n / 2^32), where n counts the samples
 * since create / tetra_chan_reset (a reset restarts n and keeps inc).  A carrier at (k + e) Fs / M lands at DC of bin k for
 * inc = e / M . 2^32 (half a bin at M = 800: 2^32 / 1600).
 *
 * The frame phasor's phase is (inc . n_m) mod 2^32, n_m = the absolute index of the frame's newest sample, and the taps' phases
 * are (inc . l) mod 2^32: both in integer arithmetic, so the result is exact at any stream position and does not depend on how
 * the capture is cut -- no accumulated floating-point phase exists.
 *
 * May be called between process calls.  It takes effect from the next call's first frame and keeps the phase reference n (no
 * reset).  hc is rebuilt in double on the host here; its upload is enqueued at the head of the next process call on that call's
 * stream, i.e. behind all work enqueued before and ahead of that call's kernel (a second set_shift while an upload still waits
 * in a stream blocks until that upload has run).  All three kernels and all three sample formats take the shift; results are held
 * to the same float32 tolerance against the double-precision definition as the un-shifted bank (2e-5 of the output's maximum;
 * measured 4.2e-7 at worst: tests/test_chan_shift.py).  TETRA_ERR_HIP / _NO_DEVICE leave the previous shift in force. */
int tetra_chan_set_shift(tetra_chan_t* h, uint32_t inc);
int tetra_chan_get_shift(tetra_chan_t* h, uint32_t* inc);
/* round(shift_hz / sample_rate_hz . 2^32) mod 2^32; negative shifts wrap (-f gives 2^32 - inc(f)).  0 for a sample rate <= 0 or a
 * shift that is not finite. */
uint32_t tetra_chan_shift_from_hz(double shift_hz, double sample_rate_hz);

/* The wideband receiver: forwards to its channeliser, same ordering rules (between process calls; from the next call's first
 * frame; tetra_wbrx_reset restarts the phase reference and keeps the shift).  tetra_wbrx_bin_power then reports the power of the
 * shifted bins. */
int tetra_wbrx_set_shift(tetra_wbrx_t* h, uint32_t inc);
int tetra_wbrx_get_shift(tetra_wbrx_t* h, uint32_t* inc);

#ifdef __cplusplus
}
#endif
#endif
