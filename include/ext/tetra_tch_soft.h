/*
 * tetra_tch_soft.h -- C ABI of the coded circuit-mode data channels TCH/4.8 and TCH/2.4 decoded from SOFT values: int8 byte rows, or
 * the soft frame decoder's ring (tetra_soft.h).  OPT-IN: nothing in tetra_tch.h or tetra_soft.h changes, and their entry points launch
 * what they launched before.
 *
 * The data channels have no CRC, so a wrongly decoded block is delivered as it is, and the 292 / 432 puncturer of TCH/4.8 erases six
 * trellis steps outright: they gain most from soft decisions.  A block is DEFINED here as the reference's own functions chained as for
 * the signalling kinds' soft route (tetra_soft.h), with the puncturers of tetra_tch.h, per block of 432 int8 soft values in type-5
 * order (positive means bit 0, negative bit 1, zero carries no decision; |value| <= 31, not checked for, as in tetra_soft.h):
 *     type5 soft --negate where tetra_scramb_bits(code) has a 1--> type4 --block_deinterleave(432, 103)--> type3
 *           --tetra_rcpc_depunct(TETRA_RCPC_PUNCT_292_432 | TETRA_RCPC_PUNCT_148_432) into a buffer of zeros--> mother code
 *           --conv_cch_decode(., ., type2_bits)--> 292 / 148 type-2 bits, one per byte
 * The tail is included, there is no CRC, and the contract is bit-exactness for ANY values in [-31, 31], the decoder's tie-break and its
 * four flush steps included.  The packed 16-bit path metrics need no renormalisation under that bound (csrc/tch_soft_core.hpp).
 *
 * Channel bit errors, errors | compared << 16 as tetra_biterr.h and tetra_soft.h define them: the decoded type-2 bits, tail included, are
 * encoded again, punctured with the kind's puncturer and interleaved; compared = the number of the 432 positions whose descrambled value
 * is not 0, errors = the number of those whose sign differs from the re-encoded bit.
 *
 * TCH/7.2 is not coded and gains nothing from soft values: every entry point here returns TETRA_ERR_ARG for it; decode it from the
 * packed frames or from byte rows of hard bits (tetra_tch.h).
 *
 * Limits.  The entry points declared here decode N = 1 only: interleaving over N = 4 or 8 blocks is tetra_tch_nblk.h's, for soft values
 * as for hard bits.  NOT built: speech (TCH/S); list decoding of TCH (there is no CRC to aim
 * at).  The chain's ring and frames are not exposed to callers, so these entry points serve a caller with a ring of its own, as
 * tetra_soft.h does; inside tetra_rx / tetra_wbrx the chain's own ring feeds the same jobs for the timeslots the host names (tetra_traffic.h).
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_TCH_SOFT_H
#define TETRA_TCH_SOFT_H

#include <stdint.h>

#include "../tetra_lmac.h"
#include "tetra_soft.h"
#include "tetra_tch.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * int8 byte rows, counted: the arguments, alignment rules and statuses of tetra_lmac_decode_tch_counted_device (tetra_tch.h), with
 *   kind          TETRA_LMAC_T_TCH_4_8 or TETRA_LMAC_T_TCH_2_4 (TETRA_LMAC_T_TCH_7_2: TETRA_ERR_ARG)
 *   d_soft        [n_blocks][in_stride] int8, 432 soft values used per row (4-byte aligned, in_stride a multiple of 4 and >= 432)
 *   d_n_blocks    NULL, or the number of rows present, read on the device; rows past it are not touched
 *   d_scramb_init the scrambling code of row j is d_scramb_init[d_init_index ? d_init_index[j] : j]
 *   d_type2       [n_blocks][out_stride] uint8 out, type2 bytes per row (4-byte aligned, out_stride a multiple of 4 and >= type2); the
 *                 padding behind a row is not written
 *   d_biterr      NULL, or [n_blocks] uint32 out (4-byte aligned): the count defined above
 * n_blocks == 0 is a no-op.  Enqueued on hip_stream, no synchronisation; the decision scratch comes from the library's stream-ordered
 * pool.
 */
int tetra_lmac_decode_tch_soft_counted_device(int kind, const int8_t* d_soft, int n_blocks, const int32_t* d_n_blocks, int in_stride,
                                              const uint32_t* d_scramb_init, const int32_t* d_init_index, uint8_t* d_type2, int out_stride,
                                              uint32_t* d_biterr, void* hip_stream);

/* Host-pointer variant (copies in/out, synchronises; device = HIP ordinal or -1 for the current one); biterr may be NULL. */
int tetra_lmac_decode_tch_soft_batch(int kind, const int8_t* soft5, int n_blocks, int in_stride, const uint32_t* scramb_init,
                                     uint8_t* type2, int out_stride, uint32_t* biterr, int device);

/*
 * tetra_lmac_decode_frames_soft_device (tetra_soft.h) that also accepts jobs of type TETRA_LMAC_T_TCH_4_8 / TETRA_LMAC_T_TCH_2_4: every
 * parameter as there, and everything that entry accepts is accepted here and produces byte for byte what it produces there.  A TCH
 * job's rows are read from the ring at the listed frames' bit numbers with the SCH/F layout -- both blocks of a TETRA_TRAIN_NORM_1
 * burst; a listed frame of another burst type decodes as a block of erasures (all soft values zero) under that frame's scrambling code,
 * with a count of 0.  blk_num is ignored; d_type2 and out_stride follow the rules of any job (8-byte aligned, out_stride a multiple of 8
 * and >= type2), d_crc_ok[row] = 1 (there is nothing to check), d_labels as for any job, d_biterr[job] as for any job.  The TCH jobs run
 * in a launch of their own behind the others on the same stream, so the kernel that decodes the signalling kinds is the kernel it was.
 * The decision scratch is the one tetra_lmac_decode_frames_workspace_bytes sizes for the same job table: the soft route needs the
 * same scratch as the hard one (a dword per step pair and row).
 * TETRA_ERR_ARG, before anything is launched or written: what tetra_lmac_decode_frames_soft_device refuses, a TETRA_LMAC_T_TCH_7_2
 * job, and a TCH job whose entry of d_rank is not NULL (there is no CRC to rescue by; the signalling jobs of the same call may have
 * ranks).  tetra_lmac_decode_frames_soft_device itself keeps refusing every TCH job.
 */
int tetra_lmac_decode_frames_soft_tch_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs,
                                             const int8_t* d_ring, uint32_t ring_size,
                                             uint32_t* const* d_biterr, int32_t* const* d_rank, int max_candidates,
                                             void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
