/*
 * tetra_gap.h -- C ABI of stream gaps: channels restarted after missing samples keep their frame timing, cell and TDMA clock.
 *
 * Every receiver here assumes an unbroken sample stream.  An SDR driver at 80 MB/s drops buffers and reports the drop as a jump in the
 * sample timestamp.  Fed the next buffer as if nothing had happened, the channeliser and the resampler filter across a seam that is not
 * there, every carrier's frame timing jumps by a non-integer number of bits, the synchroniser unlocks and relocks, and the TDMA clock,
 * which counts delivered frames, runs behind by the lost slots until that carrier's next SYNC PDU with a good CRC -- up to a multiframe
 * (1.02 s) of blocks with the wrong tn / fn / mn on a traffic carrier.  tetra_wbrx_reset throws code and clock away altogether.
 *
 * A gap is a hand-over (tetra_handover.h) in which every channel is its own donor and a known time has passed.  This DEPARTS FROM THE
 * REFERENCE like the hand-over and is opt-in: a handle that never reports a gap allocates, launches and computes what it always did.
 * The ASSIST state of the synchroniser, the apply step and the status codes are the hand-over's, unchanged.  The rule, in integer
 * arithmetic on bit positions only, per channel, for G elapsed bits (0 <= G <= 2^31 - 1), the window W and max_slots:
 *
 *   1. read the channel's own synchroniser state, hand-over fields and cell, before anything is reset.  Its anchor (a, q), a bit number
 *      and a PHY time such that the tracker gives a frame at a + 510 j the time q + j + 1:
 *        LOCKED:                          a = bitbuf_start_bitnum, q = the PHY time;
 *        ASSIST with the status PENDING:  a = the expected frame start, q = the PHY time advanced by the slot periods ASSIST has waited.
 *      Rcv = bitbuf_start_bitnum + bits_in_buf is what the channel has received, d = Rcv - a a signed difference of wrapping 32-bit numbers;
 *   2. the channel restarts exactly as tetra_rx_reset_channels_device restarts it: demodulator loops, soft ring, synchroniser, bit
 *      buffer, link figures, miss counter, bit numbering from 0;
 *   3. a channel that had an anchor and a scrambling code (scramb_init != 0): m = the smallest integer >= 0 with 510 m - (d + G) >= W,
 *      expect = 510 m - (d + G); its cell is the old one with the PHY time q advanced by m slots (m mod 4320 tetra_tdma_time_add_tn
 *      steps: the clock's period is 4320 slots); state ASSIST, status PENDING, waited 0, slots_left = max_slots;
 *   4. any other channel stays as the plain restart left it; status REFUSED.
 * With G = 0 on a LOCKED channel this is the hand-over's planting with the channel as its own donor.
 *
 * What tetra_rx_get_handover (tetra_handover.h) reports afterwards is what became of each channel: PENDING, LOCKED with its offset,
 * EXPIRED or REFUSED.
 *
 * The default window rests on a measurement (profiles/measure_gap_window.py).  A gap adds the rounding of G (at most
 * half a bit) and the restart phase of the channeliser's frame grid and of the resampler to the hand-over's displacement of 0 or 2 bits:
 * resumed carriers of a wideband handle found their frame start at -1, 0 or +1 bits from the expected one at Es/N0 11, 20 and 25 dB
 * alike, channels of a chain at a sample per bit at 0, 1 or 2; the default is twice the largest magnitude seen, rounded up to a multiple
 * of 8.  A relative error e between the capture's sample clock and the base station's moves the frame start by 36000 e bits per second
 * of gap: the 6 bits that remain of the default window cover 16.7 s at 10 ppm; a longer gap wants a wider window.
 *
 * Same conventions as tetra_rx.h: extern "C", int status, GPU only; on a machine without a HIP device every entry point returns
 * TETRA_ERR_NO_DEVICE.
 */
#ifndef TETRA_GAP_H
#define TETRA_GAP_H

#include <stdint.h>

#include "../tetra_wbrx.h"
#include "tetra_handover.h"
#include "tetra_iqcond.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TETRA_GAP_DEFAULT_WINDOW 8
#define TETRA_GAP_DEFAULT_MAX_SLOTS 72
#define TETRA_GAP_MAX_ELAPSED_BITS 2147483647 /* 2^31 - 1 bits: 16.5 hours */

/*
 * The n listed channels restart as their own heirs after elapsed_bits bits that never arrived, by the rule above.  Ordering and streams
 * are those of tetra_rx_reset_channels_device: the demodulator part on the caller's stream, the synchroniser and cell part on the chain's
 * tail stream behind the last call's tail, the next process call behind both; enqueued, never waited for (the first gap or hand-over of a
 * handle allocates the hand-over's per-channel fields and waits for the device once).  p == NULL: the defaults above.
 * TETRA_ERR_ARG: whatever tetra_rx_reset_channels_device refuses, elapsed_bits < 0 or > TETRA_GAP_MAX_ELAPSED_BITS, a window outside
 * 0 .. 127 or max_slots outside 1 .. 255; a chain that a wideband handle owns: TETRA_ERR_UNSUPPORTED.  Nothing is enqueued then.
 */
int tetra_rx_resume_channels_device(tetra_rx_t* h, const int32_t* channels, int n, int64_t elapsed_bits, const tetra_handover_params_t* p,
                                    void* hip_stream);

/*
 * n_lost >= 0 samples of the capture are missing between the last process call and the next.  Enqueues on hip_stream (the one the process
 * calls use), with no host synchronisation, the front end's state as tetra_wbrx_reset leaves it -- the channeliser's delay line and carry
 * and the resampler's delay line and output phase cleared, the retune ring cleared, the phase references of the shift and of the
 * per-carrier offsets restarted; the bin list, the shift, the offsets, the input map and the retune counts stay -- and then every carrier
 * slot resumes by the rule above with
 *   G = floor(n_lost * interp * 2 * symbolrate / (decim * decimation * samplerate) + 0.5)
 * from the handle's channeliser decimation, resampler ratio and rx.demod rates, in double; *elapsed_bits_out (may be NULL) = G.
 * Results of earlier calls stay fetchable under the `which` rules.
 * TETRA_ERR_ARG: n_lost < 0, G > TETRA_GAP_MAX_ELAPSED_BITS, parameters out of range; nothing is enqueued then.
 */
int tetra_wbrx_gap(tetra_wbrx_t* h, int64_t n_lost, const tetra_handover_params_t* p, int64_t* elapsed_bits_out, void* hip_stream);

/*
 * tetra_wbrx_process_device* for a buffer whose first sample has the driver's index first_index; fmt: TETRA_IQ_FMT_* (tetra_iqcond.h).
 * The first call of a handle (or the first after tetra_wbrx_reset) sets the stream's origin.  Later calls compare first_index with the
 * index the stream expects next (the last call's first_index + n_in):
 *   equal:   the plain process call;
 *   greater: tetra_wbrx_gap(h, first_index - expected, p, NULL, hip_stream), then the process call;
 *   smaller: an overlap -- TETRA_ERR_ARG, nothing is enqueued, the expected index stays.
 * Whatever else the process call or the gap refuses is refused before anything is enqueued, too.
 */
int tetra_wbrx_process_device_at(tetra_wbrx_t* h, const void* d_x, int fmt, int n_in, int64_t first_index, const tetra_handover_params_t* p,
                                 void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
