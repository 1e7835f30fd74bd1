/*
 * tetra_iqcond.h -- C ABI of the capture conditioning of the wideband front end: DC offset, IQ gain / phase imbalance, swapped I / Q and
 * inverted Q, cured by ONE per-sample real affine map of (I, Q) that folds into the loads the channeliser's kernels already do.
 *
 * The channeliser (tetra_chan.h) reads the SDR's samples where the DMA left them and folds the raw capture, so the capture's defects go
 * straight into the bins: a DC offset is a spur in bin 0, IQ imbalance leaves an image of every carrier at +f on -f (25 to 40 dB down
 * on zero-IF receivers: a cell 30 dB weaker than the one on its mirror bin is buried), and a capture with swapped I / Q or inverted Q
 * has its spectrum mirrored -- nothing decodes.  Everything declared here is OPT-IN: a handle that never sets a map allocates, launches
 * and computes what it always did (the un-conditioned kernels, instruction for instruction).
 *
 * The contract.  A sample is converted to binary32 first, as ever (value / 32768 for cs16, value / 128 for cs8, the complex64 as it is):
 * (xr, xi).  It then becomes, exactly (each fmaf one correctly rounded fused multiply-add),
 *
 *     yr = fmaf(m01, xi, fmaf(m00, xr, c0))
 *     yi = fmaf(m11, xi, fmaf(m10, xr, c1))
 *
 * and the channeliser's output is the output of the un-conditioned channeliser run on the stream y, bit for bit.  Sample n is conditioned
 * with the map in force in the call that DELIVERED it: the handle's delay line carries conditioned samples, and a later call with
 * another map (or none) reads them as they are.  The map acts before the frequency shift (tetra_shift.h), which lives in the taps, and
 * is independent of it.  The retune, the bin power, the resampled frames and the receive chain see conditioned data without any change
 * of their own.
 *
 * Two limits:
 *   - The map is one set of six numbers for the whole band: it corrects FREQUENCY-INDEPENDENT imbalance only.  The frequency-dependent
 *     part of a real receiver's imbalance (its two anti-alias filters differ) stays.
 *   - The estimate (tetra_iq_map_from_stats) is BLIND: it assumes that the clean capture is proper, E[z^2] = 0, which a sum of modulated
 *     carriers away from DC is.  A capture dominated by one unmodulated tone, by a carrier on DC or by a real-valued interferer is not;
 *     the estimate then removes correlation that belongs to the signal.
 * Tracking the map from call to call is not done here: estimate once (or now and then) from a stretch of the capture, and set the result.
 *
 * Same conventions as tetra_chan.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only (the solver needs none).
 */
#ifndef TETRA_IQCOND_H
#define TETRA_IQCOND_H

#include <stdint.h>

#include "../tetra_chan.h"
#include "../tetra_wbrx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* (yr, yi) = (m00 xr + m01 xi + c0, m10 xr + m11 xi + c1), evaluated as stated above.  {1, 0, 0, 1, 0, 0} is the identity, {0, 1, 1, 0, 0, 0}
 * swaps I and Q, {1, 0, 0, -1, 0, 0} inverts Q, {1, 0, 0, 1, -dI, -dQ} removes a DC offset (in the converted samples' unit, full scale = 1). */
typedef struct tetra_iq_map {
    float m00, m01, m10, m11, c0, c1;
} tetra_iq_map_t;

/* Sums over n samples (xr, xi) in the converted samples' unit: s_i = sum xr, s_q = sum xi, s_ii = sum xr^2, s_qq = sum xi^2, s_iq = sum xr xi. */
typedef struct tetra_iq_stats {
    int64_t n;
    double s_i, s_q, s_ii, s_qq, s_iq;
} tetra_iq_stats_t;

/* Sample formats of tetra_iq_stats_device: what the three tetra_chan_process_device* entry points read. */
#define TETRA_IQ_FMT_C64 0  /* complex64: interleaved float I, Q */
#define TETRA_IQ_FMT_CS16 1 /* interleaved int16 I, Q */
#define TETRA_IQ_FMT_CS8 2  /* interleaved int8 I, Q */

/*
 * Sets the map of the handle's input, or -- map == NULL -- returns it to the un-conditioned kernels.  May be called between process calls;
 * it touches nothing on the device and waits for nothing (the six numbers travel as kernel arguments), and takes effect with the next
 * process call's first new sample.  A coefficient that is not finite: TETRA_ERR_ARG, and the previous map stays.  tetra_chan_reset treats the
 * map as it treats the shift: it keeps it.  With a map set, all three kernels and all three sample formats go through it (the staged
 * kernels' complex64 input too, in place of the plain copy).
 */
int tetra_chan_set_input_map(tetra_chan_t* h, const tetra_iq_map_t* map);
/* *map = the map in force (the identity if none is set); *is_set (may be NULL) = 1 if one is set, else 0. */
int tetra_chan_get_input_map(tetra_chan_t* h, tetra_iq_map_t* map, int* is_set);

/* The wideband receiver: forwards to its channeliser, same rules (tetra_wbrx_reset keeps the map). */
int tetra_wbrx_set_input_map(tetra_wbrx_t* h, const tetra_iq_map_t* map);
int tetra_wbrx_get_input_map(tetra_wbrx_t* h, tetra_iq_map_t* map, int* is_set);

/*
 * The sums of n samples at d_x (device memory, format fmt) in one pass over the capture, into *out (HOST memory); enqueued on hip_stream
 * and waited for.  It has no handle: it runs on the calling thread's current device, which must be the one d_x lives on.  n = 0 gives zeros.
 *   cs16 / cs8: the sums are accumulated exactly, in 64-bit integers, and converted once: every field is the correctly rounded double of
 *     the exact integer sum times the power-of-two scale of the unit (2^-15 / 2^-30 for cs16, 2^-7 / 2^-14 for cs8) -- uniquely defined,
 *     whatever the order.  n <= 2^32 (TETRA_ERR_SIZE above: the sum of squares would leave 64 bits).
 *   complex64: float64 accumulation of float64 terms in a fixed order that depends on n alone: the same input and n give the same bits on
 *     every call, on every device.
 * TETRA_ERR_ARG: out == NULL, d_x == NULL with n > 0, a format other than the three; TETRA_ERR_SIZE: n < 0 (or above the integer limit);
 * TETRA_ERR_ALIGN: d_x not aligned to one sample of the format (8 / 4 / 2 bytes), as in the channeliser.
 */
int tetra_iq_stats_device(const void* d_x, int fmt, long long n, tetra_iq_stats_t* out, void* hip_stream);

/*
 * The map that removes the DC offset and makes I and Q uncorrelated and of equal power (Gram-Schmidt: I is left alone, Q is
 * decorrelated and equalised).  Host only; computed in double exactly as written, then rounded to float:
 *
 *     uI = s_i / n,  uQ = s_q / n
 *     A = s_ii / n - uI uI,   B = s_qq / n - uQ uQ,   C = s_iq / n - uI uQ
 *     r = C / A,   k = sqrt(A / (B - C C / A))
 *     m00 = 1,  m01 = 0,  c0 = -uI
 *     m10 = -(k r),  m11 = k,  c1 = k (r uI - uQ)
 *
 * For a capture I' = I + dI, Q' = g (Q cos phi + I sin phi) + dQ of a proper signal this is the exact inverse (up to the estimate's
 * noise).  TETRA_ERR_ARG where stats or map is NULL, n < 2, A <= 0 or B - C C / A <= 0 (a constant I; I and Q perfectly correlated), or a
 * result that is not finite.
 */
int tetra_iq_map_from_stats(const tetra_iq_stats_t* stats, tetra_iq_map_t* map);

#ifdef __cplusplus
}
#endif
#endif
