/*
 * tetra_wbrx.h -- C ABI of the wideband receiver: ONE SDR capture in, the decoded blocks of every selected TETRA carrier out.
 *
 * The reference plugin asks SDR++ for one VFO per carrier (src/main.cpp:75) and runs one demodulator + decoder instance on each
 * 36 ksps stream.  This handle replaces the N VFOs and N instances by the library's own stages behind one handle:
 *
 *     capture (complex64 / cs16 / cs8)  ->  channeliser (tetra_chan.h: M bins, 50 ksps each at 20 MHz / 800 / 400)
 *                                       ->  selecting resampler: the carriers' bins only, 18 / 25 -> 36 ksps
 *                                       ->  receive chain (tetra_rx.h) on [frames][n_bins] time-major frames
 *
 * so that everything behind the channeliser's FFT costs in proportion to the carriers, not to the M bins.  The resampled IQ of
 * carrier j is column bins[j] of tetra_resamp run on all M bins, bit for bit; the chain's output is then what tetra_rx gives for
 * those columns.  The handle has no per-carrier mixer: the carriers must share ONE offset from the bins' centres (k Fs / M).  That
 * offset -- zero, or the fraction of a bin that the band's raster and the SDR's tuning leave, typically half a bin -- goes into the
 * channeliser's frequency shift (tetra_wbrx_set_shift, tetra_shift.h), which costs no extra pass over the capture; a residual of a
 * few hundred hertz is the demodulator FLL's business, as before.
 *
 * Same conventions as the other headers: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, one thread per handle,
 * GPU only; every mis-sized or misaligned buffer is a status.
 */
#ifndef TETRA_WBRX_H
#define TETRA_WBRX_H

#include <stdint.h>

#include "tetra_chan.h"
#include "tetra_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tetra_wbrx_config {
    tetra_chan_config_t chan;      /* the channeliser: M, P, D, cutoff, prototype, device; max_in = the largest n_in of one call */
    int32_t interp;                /* resampler I (18) */
    int32_t decim;                 /* resampler DN (25) */
    int32_t taps_per_phase;        /* resampler T (16); prototype I*T taps, as tetra_resamp_create designs it */
    int32_t n_bins;                /* carriers to receive: 1 .. M */
    double resamp_cutoff_rel;      /* resampler prototype cutoff (1.0), as tetra_resamp_config_t.cutoff_rel */
    double resamp_kaiser_beta;     /* its Kaiser parameter (6.0) */
    const int32_t* bins;           /* [n_bins] channeliser bins in [0, M), no duplicates; carrier j = bins[j] (copied at create) */
    tetra_rx_config_t rx;          /* the receive chain.  The handle fills in three fields of rx.demod: n_channels (= n_bins),
                                      layout (TETRA_LAYOUT_TIME_MAJOR) and max_samples (from chan.max_in); each must be 0 or that
                                      value (TETRA_ERR_ARG otherwise).  rx.demod.device must be -1 or chan.device.  Every other
                                      field is the chain's own (kinds, flags, the demodulator's parameters) */
} tetra_wbrx_config_t;

typedef struct tetra_wbrx tetra_wbrx_t;

/* 800 bins at 20 MHz (M 800, P 8, D 400, as tetra_chan_default_config) -> 18 / 25, 16 taps -> the plugin's demodulator parameters,
 * every block kind decoded.  n_bins = 0 and bins = NULL: the caller supplies the bin list. */
int tetra_wbrx_default_config(tetra_wbrx_config_t* cfg);
/* TETRA_ERR_ARG: a bin outside [0, M), a duplicate bin, n_bins < 1 or > M, a contradictory rx.demod field (above); the channeliser's,
 * resampler's and chain's own refusals as they return them. */
int tetra_wbrx_create(const tetra_wbrx_config_t* cfg, tetra_wbrx_t** out);
int tetra_wbrx_destroy(tetra_wbrx_t* h);
/* Clears the channeliser's and the resampler's delay lines and resets the chain (tetra_rx_reset).  Synchronises. */
int tetra_wbrx_reset(tetra_wbrx_t* h);

/* d_x: n_in capture samples on the device, read IN PLACE by the work enqueued here (it must stay untouched until that has run):
 * complex64 (8-byte aligned), cs16 / cs8 interleaved I, Q (4- / 2-byte aligned, value = integer / 32768 / 128): TETRA_ERR_ALIGN
 * otherwise.  n_in <= chan.max_in (TETRA_ERR_SIZE).  Enqueues on hip_stream: channeliser -> selecting resampler ->
 * tetra_rx_process_device on the resampled frames, and returns without synchronising.  Every call is exactly ONE chain call, also
 * when it yields no resampled frame (n_in < D), so the chain's which = 0 / 1 name wideband calls; the chain's limit of two calls in
 * flight carries over.  The delay lines are carried across calls: the results do not depend on how the capture is cut. */
int tetra_wbrx_process_device(tetra_wbrx_t* h, const float* d_x, int n_in, void* hip_stream);
int tetra_wbrx_process_device_cs16(tetra_wbrx_t* h, const int16_t* d_x, int n_in, void* hip_stream);
int tetra_wbrx_process_device_cs8(tetra_wbrx_t* h, const int8_t* d_x, int n_in, void* hip_stream);
/* Host-pointer variants: copy the samples in (synchronously, after the previous call's channeliser has read its copy), then the
 * same on the null stream. */
int tetra_wbrx_process(tetra_wbrx_t* h, const float* x, int n_in);
int tetra_wbrx_process_cs16(tetra_wbrx_t* h, const int16_t* x, int n_in);

/* The receive chain inside, for tetra_rx_fetch, _rows_device, _get_cell, _get_sync_state, _bits_device, _stage_ms, _wait,
 * tetra_rx_demod and the whole delivery of tetra_rx_out.h.  A block's `channel` is the carrier's index into the bin list.  The
 * caller must not process, reset or destroy it through tetra_rx_*: the wideband handle owns it. */
tetra_rx_t* tetra_wbrx_rx(tetra_wbrx_t* h);
/* The bin list, in the order given at create: out [n_bins]. */
int tetra_wbrx_bins(tetra_wbrx_t* h, int32_t* out);
/* The resampled carrier IQ [*n_frames][n_bins] complex64 (time-major, what the demodulator read) of the latest (which = 0) or the
 * previous (1) call, where it is.  Ordered like tetra_rx_bits_device: hip_stream is made to wait for the resampler of that call.
 * Valid until the next-but-one call.  Before the first call / which = 1 before the second: *n_frames = 0. */
int tetra_wbrx_frames_device(tetra_wbrx_t* h, int which, const float** d_frames, int* n_frames, void* hip_stream);
/* out [M]: the mean of |X_k|^2 over the channeliser frames of the latest call, for every bin k (zeros when that call had none, or
 * before the first).  Waits for that call's channeliser, reduces on the device (on demand: the calls themselves do no extra work),
 * copies M floats back. */
int tetra_wbrx_bin_power(tetra_wbrx_t* h, float* out);
/* GPU time (ms) of the latest call's channeliser kernel (ms[0]) and resampler kernel (ms[1]), from HIP events on its stream.  The
 * chain's stages: tetra_rx_stage_ms(tetra_wbrx_rx(h), ...). */
int tetra_wbrx_stage_ms(tetra_wbrx_t* h, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
