/*
 * tetra_biterr.h -- C ABI of the channel bit-error count of the convolutionally coded blocks (SB1, SB2, NDB, SCH/HU, SCH/F).
 *
 * The lower-MAC decoder (tetra_lmac.h) reports one bit of link quality per block, the CRC verdict.  Every TETRA receiver also shows a
 * channel bit-error estimate: it encodes the decoded block again and compares the result with what it received.  The entry points
 * declared here do that inside the decode kernels, where the decoded bits and the received block are still in the lane when the
 * traceback ends; nothing is read again from memory.  They are OPT-IN and change nothing unless used: a call without a count array
 * launches the kernels the entry points of tetra_lmac.h launch and writes the same bytes.
 *
 * Definition, pinned on the reference's own encoder primitives (src/decoder/src/lower_mac/).  For a block of kind t
 * (tetra_lmac_blk_param: type345_bits, type2_bits, interleave_a) let d[0 .. type2_bits) be the decoded type-2 bits as the decoder
 * writes them -- all of them, the four tail positions included (on a noisy block the tail is not always zero).  Encode d as a
 * transmitter would: conv_enc_init / conv_enc_input from the all-zero state, get_punctured_rate(TETRA_RCPC_PUNCT_2_3),
 * block_interleave(type345_bits, a), tetra_scramb_bits with the block's scrambling code (SCRAMB_INIT for SB1).  That gives
 * e[0 .. type345_bits), the type-5 bits a transmitter would have sent for d.  Then
 *     compared = the received positions that carry a decision
 *                byte rows and packed frames: every position whose descrambled byte is not the erasure 0xff (rows of 0 / 1 bytes and
 *                frames: type345_bits); soft values: every position whose value is not 0
 *     errors   = the compared positions whose received hard bit differs from e
 *                byte rows: a descrambled byte 0 is a 0, any other a 1 (viterbi.c:12-23); soft values: 1 iff negative
 * and the value per block is errors | compared << 16, one uint32 (both at most 432).  A listed frame whose burst type does not carry
 * the kind decodes as the all-zero block and counts as the definition says for that input: no special case.
 *
 * errors is the distance from the received word to the DECODED codeword.  It equals the number of channel errors while the decoder
 * decodes correctly, so it is an ESTIMATE THAT IS MEANINGFUL FOR BLOCKS WITH A GOOD CRC: on pure noise the decoder finds a codeword
 * about 35 of 432 bits away, whatever was sent.  The AACH (TETRA_TPSAP_T_BBK) is not convolutionally coded; its own distance is in
 * tetra_aach.h.
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_BITERR_H
#define TETRA_BITERR_H

#include <stdint.h>

#include "../tetra_lmac.h"
#include "../tetra_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TETRA_BITERR_ERRORS(v) ((uint32_t)(v) & 0xffffu)
#define TETRA_BITERR_COMPARED(v) ((uint32_t)(v) >> 16)

/*
 * tetra_lmac_decode_counted_device with the counts: every argument as there, plus
 *   d_biterr  [n_blocks] uint32 out (4-byte aligned): errors | compared << 16 per row; rows past the count (*d_n_blocks) are not touched.
 *             NULL: exactly tetra_lmac_decode_counted_device.  With TETRA_TPSAP_T_BBK a non-NULL pointer is TETRA_ERR_ARG.
 * Both routes of the decoder's front end count (tetra_lmac_debug_force_byte_route); they give the same values on the same rows.
 */
int tetra_lmac_decode_counted_biterr_device(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                            const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                            int32_t* d_crc_ok, uint32_t* d_biterr, void* hip_stream);

/* Host-pointer variant: tetra_lmac_decode_batch plus biterr [n_blocks] (NULL: exactly that function). */
int tetra_lmac_decode_batch_biterr(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                   uint8_t* type2, int out_stride, int32_t* crc_ok, uint32_t* biterr, int device);

/*
 * tetra_lmac_decode_frames_device with the counts: src, jobs and n_jobs as there, plus
 *   d_biterr  [n_jobs] device pointers (the array itself is host memory), entry i = [jobs[i].max_rows] uint32 out (4-byte aligned),
 *             written for the rows the job decodes.  An entry may be NULL: that job does not count.  It must be NULL for a BBK job
 *             (with or without TETRA_LMAC_JOB_RM3014), else TETRA_ERR_ARG.  A NULL array: exactly tetra_lmac_decode_frames_device.
 * Rows, verdicts and labels are those of tetra_lmac_decode_frames_device.
 */
int tetra_lmac_decode_frames_biterr_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, uint32_t* const* d_biterr,
                                           void* hip_stream);

/*
 * The receive chain: TETRA_RX_FLAG_BITERR in tetra_rx_config_t.flags (tetra_rx.h; through cfg.rx also for tetra_wbrx_create, whose chain
 * tetra_wbrx_rx hands out) makes the chain's decode launches count, with the packed frames or -- with TETRA_RX_FLAG_SOFT -- the soft
 * values as the received word.  The handle then keeps one uint32 per row for each coded kind it decodes, double buffered like the
 * results (4 bytes per row and kind), and the link figures below.  The tetra_rx_out.h delivery format is unchanged; the counts and the
 * link figures come with a call's rows, without a host synchronisation, as a column and a per-channel table of an extended delivery
 * (tetra_rx_out_ext.h: TETRA_RX_OUT_EXT_ROW_BITERR, TETRA_RX_OUT_EXT_CHAN_LINK), or through the blocking calls here.
 *
 * tetra_rx_fetch_biterr: errors | compared << 16 of every row of a coded kind of the latest (which = 0) or previous (1) call, in
 * tetra_rx_fetch's order.
 *   out      [capacity] uint32 host, may be NULL
 *   *n_rows  rows available; more than capacity with out != NULL: TETRA_ERR_SIZE and nothing is copied
 * TETRA_ERR_UNSUPPORTED if the handle was created without the flag, for TETRA_RX_KIND_BBK, or for a kind the handle does not decode.
 * Before the first call / which = 1 before the second: 0 rows.
 */
int tetra_rx_fetch_biterr(tetra_rx_t* h, int which, int kind, uint32_t* out, int capacity, int* n_rows);
/* The same rows where they are: *d_biterr [rows] uint32 on the device, row for row beside tetra_rx_rows_device's (whose d_n_rows counts
 * them); hip_stream is made to wait for the call's tail.  Valid until the next-but-one process call.  Statuses as tetra_rx_rows_device. */
int tetra_rx_biterr_device(tetra_rx_t* h, int which, int kind, const uint32_t** d_biterr, void* hip_stream);

/*
 * Link figures per channel, kept on the device and accumulated by a small kernel in the tail of every call, behind the decode launches,
 * over every coded kind the handle decodes (SB1 included).  bit_errors / bits is the channel bit-error rate estimate: both are summed
 * over the blocks with a GOOD CRC only, where the count is the number of channel errors.
 * tetra_rx_reset zeroes them; tetra_rx_reset_channels_device (tetra_retune.h) zeroes the listed channels' in stream order, and through
 * it tetra_wbrx_retune those of the carrier slots it moves.
 */
typedef struct tetra_rx_link {
    uint64_t bits;           /* sum of `compared` over CRC-good coded blocks */
    uint64_t bit_errors;     /* sum of `errors` over the same blocks */
    uint32_t blocks;         /* coded blocks seen, over all coded kinds the handle decodes, SB1 included */
    uint32_t blocks_crc_bad;
} tetra_rx_link_t;
/* Channels first .. first + count - 1; waits for the latest call's tail, like tetra_rx_get_cell.  TETRA_ERR_UNSUPPORTED without the flag. */
int tetra_rx_get_link(tetra_rx_t* h, int first, int count, tetra_rx_link_t* out);

#ifdef __cplusplus
}
#endif
#endif
