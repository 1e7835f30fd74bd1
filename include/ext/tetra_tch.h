/*
 * tetra_tch.h -- C ABI of the circuit-mode data channels of the lower MAC: TCH/7.2, TCH/4.8 and TCH/2.4 (EN 300 392-2 8.2.3.1.5 / .6,
 * 8.3.1).  OPT-IN: nothing in tetra_lmac.h changes, and a call that names none of the kinds below launches what it launched before.
 *
 * The reference decodes no traffic channel, but it holds everything the data channels need: the puncturers punct_292_432 and
 * punct_148_432 (src/decoder/src/lower_mac/tetra_conv_enc.c:148-164, i_func_292 / i_func_148 at :120-128, never called there) over the
 * K = 5 rate-1/4 mother code and the (432, 103) block interleaver that SCH/F uses.  A block of one of these kinds is DEFINED here as the
 * reference's own functions chained in the order of tp_sap_udata_ind (tetra_lower_mac.c:184-214), per row:
 *     type5 --tetra_scramb_bits(row's code)--> type4 --block_deinterleave(432, 103)--> type3
 *           --tetra_rcpc_depunct(TETRA_RCPC_PUNCT_292_432 | TETRA_RCPC_PUNCT_148_432) into a buffer of 0xff bytes--> mother code
 *           --viterbi_dec_sb1_wrapper(., ., type2_bits)--> type2_bits decoded bits, one per byte
 * and the contract is that of tetra_lmac.h: bit-exact for ANY input bytes (after descrambling a byte 0 is a strong 0, 0xff an erasure,
 * anything else a strong 1), the decoder's tie-break (even predecessor wins) and its four zero-metric flush steps included.  TCH/7.2 is
 * not coded: its 432 descrambled bytes come back masked to their low bit.  There is no CRC on any of the three.
 *
 *     kind      type345  type2  type1  interleave a   step patterns (g1 g2 g3 g4, 1 = sent)
 *     TCH/7.2     432     432    432       0           --
 *     TCH/4.8     432     292    288      103          1100 x 146, 1000 x 140, 0000 x 6
 *     TCH/2.4     432     148    144      103          1110 x 136, 1100 x 12
 * type2 includes the four tail bits (tetra_conv_enc.c:262-263).  The 292 / 432 puncturer erases six trellis steps completely, so a single
 * channel error can already lose a TCH/4.8 block: that is the code, and it is reproduced, not mended.
 *
 * Limits.  The entry points declared here decode N = 1 only; interleaving over N = 4 or 8 blocks (EN 300 392-2 8.2.4.2) is
 * tetra_tch_nblk.h's, with entry points of its own over a pool of received bursts and a window table.  Which (carrier, timeslot) carries circuit-mode
 * data, and at which rate, is upper-MAC knowledge that stays on the host: it lists those slots' frames and hands them to a TCH job, or
 * names the timeslots to tetra_rx / tetra_wbrx, which then route them to these jobs themselves (tetra_traffic.h).  No speech (TCH/S).  Soft-decision decoding of TCH/4.8
 * and TCH/2.4 is tetra_tch_soft.h's, with entry points of its own; the ones declared here read hard bits.
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_TCH_H
#define TETRA_TCH_H

#include <stdint.h>

#include "../tetra_lmac.h"
#include "tetra_biterr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Block kinds beside TETRA_TPSAP_T_*: low-byte values, clear of the job flags 0x100 / 0x200 and of bits 16..25. */
enum {
    TETRA_LMAC_T_TCH_7_2 = 8,
    TETRA_LMAC_T_TCH_4_8 = 9,
    TETRA_LMAC_T_TCH_2_4 = 10
};

/* The table above (have_crc16 = 0).  TETRA_ERR_ARG for any other kind. */
int tetra_lmac_tch_blk_param(int kind, tetra_lmac_blk_param_t* out);

/*
 * Byte rows, counted: the arguments, alignment rules and statuses of tetra_lmac_decode_counted_biterr_device without d_crc_ok.
 *   kind          TETRA_LMAC_T_TCH_*
 *   d_type5       [n_blocks][in_stride] uint8, 432 bytes used per row (4-byte aligned, in_stride a multiple of 4 and >= 432)
 *   d_n_blocks    NULL, or the number of rows present, read on the device; rows past it are not touched
 *   d_scramb_init the scrambling code of row j is d_scramb_init[d_init_index ? d_init_index[j] : j]
 *   d_type2       [n_blocks][out_stride] uint8 out, type2 bytes per row (4-byte aligned, out_stride a multiple of 4 and >= type2)
 *   d_biterr      NULL, or [n_blocks] uint32 out (4-byte aligned): errors | compared << 16 as tetra_biterr.h defines it -- the decoded
 *                 type-2 bits, tail included, encoded again from the all-zero state, punctured with the kind's puncturer, interleaved and
 *                 held against the descrambled received word over all 432 positions (those that are no erasure are compared).  The only
 *                 quality figure a block without a CRC has.  TETRA_ERR_ARG with TETRA_LMAC_T_TCH_7_2, which is not coded.
 * Rows of plain 0 / 1 bytes take the decoder's packed route, anything else its byte route (tetra_lmac_debug_force_byte_route); the
 * results are the same bit for bit.  n_blocks == 0 is a no-op.  Enqueued on hip_stream, no synchronisation; the decision scratch comes
 * from the library's stream-ordered pool.
 */
int tetra_lmac_decode_tch_counted_device(int kind, const uint8_t* d_type5, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                         const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                         uint32_t* d_biterr, void* hip_stream);

/* Host-pointer variant (copies in/out, synchronises; device = HIP ordinal or -1 for the current one); biterr may be NULL. */
int tetra_lmac_decode_tch_batch(int kind, const uint8_t* type5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                uint8_t* type2, int out_stride, uint32_t* biterr, int device);

/*
 * Packed frames: tetra_lmac_decode_frames_device, tetra_lmac_decode_frames_biterr_device and tetra_lmac_decode_frames_workspace_bytes
 * accept a job whose type is one of the kinds above (blk_num is ignored).  Its rows are cut from the listed frames with the SCH/F
 * layout -- both blocks of a TETRA_TRAIN_NORM_1 burst; a listed frame of another burst type decodes as the all-zero block.  d_type2 and
 * out_stride follow the rules of any job (8-byte aligned, out_stride a multiple of 8 and >= type2), d_crc_ok[row] = 1 (there is nothing
 * to check, as the reference reports for the AACH), d_labels as for any job, counts as tetra_biterr.h (not for TCH/7.2).  TCH jobs and
 * the kinds of tetra_lmac.h may be mixed in one call: the TCH jobs run in a launch of their own behind the others on the same stream,
 * so the kernel that decodes the signalling kinds is the kernel it was.  The soft frame decoder (tetra_soft.h; tetra_tch_soft.h declares the entry
 * that takes TCH jobs on soft values) and the list decoder (tetra_list.h) return TETRA_ERR_ARG for a TCH job; the entry points of tetra_lmac.h that take one kind per call return for the values
 * 8..10 what they always returned.
 */

#ifdef __cplusplus
}
#endif
#endif
