/*
 * tetra_list.h -- C ABI of the CRC-aided list decoding of CRC-failed blocks (SB1, SB2, NDB, SCH/HU, SCH/F).
 *
 * Every convolutionally coded block carries a 16-bit CRC.  The lower-MAC decoder (tetra_lmac.h) uses it only to say "bad" about the single
 * maximum-likelihood path; when that path fails, the transmitted codeword is very often the second or third best one.  The entry
 * points declared here try a few runner-up paths against the CRC (list Viterbi decoding, Seshadri and Sundberg), for the FAILED rows
 * only, in launches of their own behind the decode launch.  They are OPT-IN and DEPART FROM THE REFERENCE, which has no such step: a
 * call without a rank array launches exactly what the entry points of tetra_lmac.h launch and writes the same bytes.
 *
 * Definition.  A block has N = type2_bits + 4 trellis steps (four flush steps on zero input).  The decoder's result is the ML path:
 * the traceback from state 0 after the flush steps, ties keeping the even predecessor.  Let s_t be its state after step t.
 *   margin        D_t = the add-compare-select difference into state s_t at step t -- the path through the even predecessor minus the
 *                 path through the odd one, in the units of the route's branch metrics (received bits and erasures as +-127 / 0 in
 *                 units of 127 on byte rows and frames, raw 6-bit values on soft values) --, Delta_t = |D_t|.
 *   candidate(t)  the traceback from state 0 with the single decision at (step t, state s_t) inverted and every other decision as
 *                 stored: the best path that merges into the ML path at step t.
 *   order         ascending Delta_t, ties by ascending t, over all N steps (the first steps and the flush steps take part; a
 *                 candidate that leaves the CRC-covered bits unchanged fails again and uses up its place).
 *   rescue        for a row whose ML path fails the CRC the first T candidates (T = max_candidates, 1..8; TETRA_LIST_DEFAULT_CANDIDATES
 *                 = 4) are tried in that order; the first whose CRC over type1_bits + 16 bits is good wins: all type2_bits of it are
 *                 written to the row, crc_ok becomes 1 (also in the row's label), rank = its 1-based place in the order.  If none
 *                 passes, the row, its verdict and its label stay byte for byte what the decoder wrote and rank = -1.  Rows whose
 *                 ML path passed get rank = 0.  Rows past a device-side count are not touched.
 * Both routes of the byte-row front end (tetra_lmac_debug_force_byte_route; 0xff erasures) and packed frames give the same margins and
 * so the same rescued rows.
 *
 * THE TRADE.  A wrong candidate passes a 16-bit CRC by accident with probability 2^-16, so every tried candidate adds that much to the
 * false-accept rate of a failed block: at most T * 2^-16 per failed block, against 2^-16 for the ML path alone.  `rank` is there so
 * that a consumer can discard rescued rows (rank > 0), keep only early ranks, or run with a smaller T.
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_LIST_H
#define TETRA_LIST_H

#include <stdint.h>

#include "../tetra_lmac.h"
#include "../tetra_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TETRA_LIST_MAX_CANDIDATES 8
#define TETRA_LIST_DEFAULT_CANDIDATES 4

/*
 * tetra_lmac_decode_counted_device with the rescue: every argument as there, plus
 *   max_candidates  T, 1..8 (else TETRA_ERR_ARG when d_rank is given)
 *   d_rank          [n_blocks] int32 out (4-byte aligned, else TETRA_ERR_ALIGN): 0 / rank / -1 per row as defined above; rows past the count
 *                   (*d_n_blocks) are not touched.  NULL: exactly tetra_lmac_decode_counted_device (max_candidates is not looked at).
 *                   With TETRA_TPSAP_T_BBK a non-NULL pointer is TETRA_ERR_ARG.
 * d_type5 is read again by the rescue: it must stay valid and unchanged until the call's work on the stream is done (as d_type2).
 */
int tetra_lmac_decode_counted_list_device(int type, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                          const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                          int32_t* d_crc_ok, int max_candidates, int32_t* d_rank, void* hip_stream);

/* Host-pointer variant: tetra_lmac_decode_batch plus max_candidates and rank [n_blocks] (NULL: exactly that function). */
int tetra_lmac_decode_batch_list(int type, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                 uint8_t* type2, int out_stride, int32_t* crc_ok, int max_candidates, int32_t* rank, int device);

/*
 * tetra_lmac_decode_frames_device with the rescue: src, jobs and n_jobs as there, plus
 *   max_candidates  T for every job that has ranks
 *   d_rank          [n_jobs] device pointers (the array itself is host memory), entry i = [jobs[i].max_rows] int32 out (4-byte aligned),
 *                   written for the rows the job decodes.  An entry may be NULL: that job is not rescued.  It must be NULL for a BBK job
 *                   (with or without TETRA_LMAC_JOB_RM3014), else TETRA_ERR_ARG.  A NULL array: exactly tetra_lmac_decode_frames_device.
 * A rescued row's label (jobs[i].d_labels) has crc_ok = 1; every other field of it is what the decoder wrote.
 */
int tetra_lmac_decode_frames_list_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, int max_candidates,
                                         int32_t* const* d_rank, void* hip_stream);

/*
 * The receive chain: TETRA_RX_FLAG_LIST in tetra_rx_config_t.flags (tetra_rx.h; through cfg.rx also for tetra_wbrx_create, whose chain
 * tetra_wbrx_rx hands out) puts the rescue behind the chain's decode launches, on the packed frames or -- with TETRA_RX_FLAG_SOFT -- the
 * soft values.  SB1 rows are rescued in front of the SYNC tracker, so a rescued SYNC PDU sets the scrambling code and the clock of its
 * burst and of what follows; the other coded kinds are rescued in front of the link figures (TETRA_RX_FLAG_BITERR: a rescued row's count is
 * taken again on the rescued codeword) and of the event that ends the tail.  Rows, labels (crc_ok = 1 for a rescued row) and the
 * tetra_rx_out.h delivery -- its TETRA_RX_OUT_CRC_GOOD selection included -- see rescued rows as good rows; the format is unchanged, and the
 * ranks come with the rows as a column of an extended delivery (tetra_rx_out_ext.h, TETRA_RX_OUT_EXT_ROW_LIST_RANK) -- which rows were
 * rescued, beside the rows themselves -- or through the blocking fetch here.  The handle keeps one int32 per row for each coded kind it decodes, double buffered
 * like the results (8 bytes per row and kind).
 *
 * tetra_rx_set_list_candidates: T for the calls that follow (1..8, else TETRA_ERR_ARG; a new handle has TETRA_LIST_DEFAULT_CANDIDATES).
 * TETRA_ERR_UNSUPPORTED if the handle was created without the flag.
 */
int tetra_rx_set_list_candidates(tetra_rx_t* h, int max_candidates);
/*
 * tetra_rx_fetch_list_rank: the rank (0 = the decoder's own path passed, k >= 1 = rescued by candidate k, -1 = failed and not rescued) of
 * every row of a coded kind of the latest (which = 0) or previous (1) call, in tetra_rx_fetch's order.
 *   out      [capacity] int32 host, may be NULL
 *   *n_rows  rows available; more than capacity with out != NULL: TETRA_ERR_SIZE and nothing is copied
 * TETRA_ERR_UNSUPPORTED if the handle was created without the flag, for TETRA_RX_KIND_BBK, or for a kind the handle does not decode.
 * Before the first call / which = 1 before the second: 0 rows.
 */
int tetra_rx_fetch_list_rank(tetra_rx_t* h, int which, int kind, int32_t* out, int capacity, int* n_rows);
/* The same rows where they are: *d_rank [rows] int32 on the device, row for row beside tetra_rx_rows_device's (whose d_n_rows counts them);
 * hip_stream is made to wait for the call's tail.  Valid until the next-but-one process call.  Statuses as tetra_rx_rows_device. */
int tetra_rx_list_rank_device(tetra_rx_t* h, int which, int kind, const int32_t** d_rank, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
