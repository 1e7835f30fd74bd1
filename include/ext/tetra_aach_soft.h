/*
 * tetra_aach_soft.h -- C ABI of the AACH's soft-decision decoding: exact maximum-likelihood (ML) decoding of the shortened (30,14)
 * Reed-Muller code (tetra_aach.h) on soft values, the one block the soft route of ext/tetra_soft.h left on hard bits.
 *
 * OPT-IN: nothing declared here changes a caller that does not use it.
 *
 * The definition.  Input per block: 30 soft values y[0..29] after descrambling by sign, int8 with |y| <= 31, positive = bit 0,
 * zero = an erasure (the ring's convention, ext/tetra_soft.h).  For codeword c, corr(c) = sum of y[i] * (1 - 2 c[i]).  The codewords
 * are rm3014_encode(info), info = 0..16383 (word format of tetra_aach.h: information bits in bits 29..16, parity in 15..0).
 *     best     the codeword with the largest corr; ties go to the smallest info
 *     margin   (corr(best) - the largest corr among all OTHER codewords) / 2: 0..930, 0 = a tie (the difference is always even)
 *     dist     the positions with y[i] != 0 whose sign disagrees with best: 0..30
 *     verdict  crc_ok = 1 iff margin >= min_margin; min_margin >= 1, default 1 = a unique ML codeword
 * All arithmetic is integer and exact.  Row format (32 bytes per row, as with TETRA_LMAC_JOB_RM3014):
 *     bytes 0..29   best's bits, one per byte, ALWAYS (there is no fall-back to the received bits)
 *     byte 30       dist
 *     byte 31       min(margin, 255)
 * The search is a dense int8 product of the blocks' values against the 16384 x 30 matrix of +-1 on gfx950's matrix cores
 * (v_mfma_i32_32x32x32_i8), 32 blocks per wavefront, with the arg-max, the runner-up and the tie rule in one integer key per product;
 * the matrix is generated in the kernel from the code's generator (no table in memory).
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_AACH_SOFT_H
#define TETRA_AACH_SOFT_H

#include <stdint.h>

#include "../tetra_aach.h"
#include "tetra_soft.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TETRA_AACH_SOFT_MAX_MARGIN 930

/*
 * The bare primitive on n rows of soft values:
 *   d_soft       [n][soft_stride] int8 on the device, the first 30 of a row used (descrambled already); 4-byte aligned, soft_stride a
 *                multiple of 4 and >= 32 (else TETRA_ERR_ALIGN / TETRA_ERR_ARG).  |value| <= 31 is not checked for.
 *   d_out_words  [n] uint32 out: best's codeword           (4-byte aligned)
 *   d_dist       [n] uint8 out:  dist
 *   d_margin     [n] uint16 out: margin, not saturated      (2-byte aligned)
 * Any of the three out pointers may be NULL.  Enqueued on hip_stream of the current device, no synchronisation.  n == 0 is a no-op,
 * n < 0 TETRA_ERR_ARG.
 */
int tetra_lmac_rm3014_soft_decode_device(const int8_t* d_soft, int n, int soft_stride, uint32_t* d_out_words, uint8_t* d_dist,
                                         uint16_t* d_margin, void* hip_stream);

/*
 * The frame decoder: OR TETRA_LMAC_JOB_RM3014_SOFT into tetra_lmac_job_t.type of a TETRA_TPSAP_T_BBK job handed to
 * tetra_lmac_decode_frames_soft_device (ext/tetra_soft.h), and its rows, d_crc_ok and the labels' crc_ok follow the definition above: the
 * frame's 30 AACH positions (SYNC: one piece, NORM_1 / NORM_2: two) are read from the ring at the frame's bit number and descrambled by
 * sign with the frame's code; a listed frame of another burst type is 30 erasures (info 0, margin 0, crc_ok 0).  out_stride >= 32.
 * TETRA_LMAC_JOB_AACH_MIN_MARGIN(m) ORed in as well puts min_margin m (1..930) into bits 16..25 of the type; 0 (absent) means 1.  The
 * job struct keeps its layout.  Every other job of the call is decoded exactly as without this one; the search runs as a launch of its
 * own behind the call's decode launch and needs no workspace.
 * TETRA_ERR_ARG, before anything is launched or written:
 *   the flag in any other frame entry point (tetra_lmac_decode_frames_device, _biterr_device, _list_device);
 *   the flag on a type other than TETRA_TPSAP_T_BBK, or together with TETRA_LMAC_JOB_RM3014;
 *   the flag on a job that has a d_biterr or d_rank entry (the AACH is not convolutionally coded and has no CRC);
 *   a min_margin above 930, or min_margin bits on a job without the flag;
 *   as before, a BBK job WITHOUT the flag in tetra_lmac_decode_frames_soft_device.
 */
#define TETRA_LMAC_JOB_RM3014_SOFT 0x200
#define TETRA_LMAC_JOB_AACH_MIN_MARGIN(m) (((m) & 0x3ff) << 16)

/*
 * The receive chain: TETRA_RX_FLAG_AACH_SOFT (1024, tetra_rx.h) makes the chain's separate AACH launch under TETRA_RX_FLAG_SOFT the job
 * above.  It NEEDS TETRA_RX_FLAG_SOFT and REFUSES TETRA_RX_FLAG_AACH_RM3014 (TETRA_ERR_ARG at create) and composes with every other
 * flag.  tetra_rx_fetch(TETRA_RX_KIND_BBK) and tetra_rx_rows_device return the rows above and the verdict, the delivery with
 * TETRA_RX_OUT_CRC_GOOD keeps the accepted rows, and tetra_rx_fetch_aach_dist and the extended delivery's AACH_DIST column answer
 * with byte 30.  The margin has no column in the extended delivery: it would change the layout of ext/tetra_rx_out_ext.h; a consumer
 * that wants it takes byte 31 of tetra_rx_rows_device's rows, or the blocking fetch below.  A handle without the flag allocates,
 * launches and computes exactly what it did before the flag existed.
 *
 * tetra_rx_set_aach_min_margin: min_margin 1..930 for the handle's next tetra_rx_process call on (default 1); anything else is
 *   TETRA_ERR_ARG, a handle without the flag TETRA_ERR_UNSUPPORTED.
 * tetra_rx_fetch_aach_margin: byte 31 of every BBK row (the margin saturated at 255) of the latest (which = 0) or previous (1) call, in
 *   tetra_rx_fetch's order; shape and statuses as tetra_rx_fetch_aach_dist (tetra_aach.h), TETRA_ERR_UNSUPPORTED without the flag.
 */
int tetra_rx_set_aach_min_margin(tetra_rx_t* h, int min_margin);
int tetra_rx_fetch_aach_margin(tetra_rx_t* h, int which, uint16_t* margin, int capacity, int* n_rows);

#ifdef __cplusplus
}
#endif
#endif
