/*
 * tetra_tch_nblk.h -- C ABI of the coded circuit-mode data channels TCH/4.8 and TCH/2.4 interleaved over N = 1, 4 or 8 blocks
 * (EN 300 392-2 8.2.4.2), from hard bits and from soft values.  OPT-IN: nothing in tetra_tch.h or tetra_tch_soft.h changes, and their
 * entry points launch what they launched before.
 *
 * N is a parameter of the call that the network chooses.  With N = 4 or 8 a type-3 block is spread over N consecutive bursts of its
 * traffic slot, so that one lost, stolen or faded burst costs each of N blocks 432 / N of its bits, not one block all of them; the data
 * channels have no CRC and their puncturers erase whole trellis steps, so that is where they pay off.
 *
 * Transmitter (the clause).  For M type-3 blocks of 432 bits,
 *     b'3(m, k) = b3(m - j, j + 1 + i N)  for 1 <= m - j <= M, else 0,
 *     j = (k - 1) div (432 / N),  i = (k - 1) mod (432 / N),  k = 1 .. 432,  m = 1 .. M + N - 1,
 * then each B'3(m) goes through the (432, 103) block interleaver and the scrambler.
 *
 * Receiver, which is what is built, 0-based, per output block b with a window w[0 .. N) of received rows, P = 432 / N.  For p = 0 .. 431:
 *     j = p mod N,  i = p div N,  r = w[j],  t = (103 (j P + i + 1)) mod 432
 *     type3[p] = the descrambled value of received row r at type-4 position t; an erasure if row r is lost
 * (block_deinterleave(432, 103) of the reference is b'3[k0] = type4[(103 (k0 + 1)) mod 432], which is where t comes from).  Then the
 * chains of tetra_tch.h and tetra_tch_soft.h run unchanged:
 *     hard:  tetra_rcpc_depunct(292_432 | 148_432) onto 0xff, then viterbi_dec_sb1_wrapper.  The byte rule is tetra_tch.h's: after
 *            descrambling 0 is a strong 0, 0xff an erasure, anything else a strong 1.  A lost row is 0xff throughout.
 *     soft:  tetra_rcpc_depunct onto zeros, then conv_cch_decode.  Values are int8 in [-31, 31] (not checked for), negated where the
 *            scrambling sequence of their received row has a 1.  A lost row is zeros.
 * N = 1 with w[0] = b is tetra_tch.h / tetra_tch_soft.h, bit for bit.  The contract is theirs: bit-exact for ANY input bytes or values,
 * the decoder's tie-break and its four flush steps included; the packed 16-bit path metrics need no renormalisation, since a gathered
 * block still has 432 values of magnitude <= 31 (csrc/tch_soft_core.hpp).
 * The reference has no code for the diagonal step, and no second implementation pins it: the clause above is the definition.  The tests
 * hold the receiver's gather against a transmitter written from the clause independently of it.
 *
 * Channel bit errors, errors | compared << 16, in the type-3 domain: the decoded type-2 bits, tail included, are encoded again and
 * punctured, then held against type3[p]; compared = the positions that are no erasure (not 0xff hard, not 0 soft), errors = those whose
 * bit or sign differs.  A lost row lowers `compared` by 432 / N.  For N = 1 these are the words of tetra_tch.h / tetra_tch_soft.h.
 *
 * Why a window table: a stream's last N - 1 bursts belong to the next call as well, bursts get lost or stolen, and many streams of
 * different length share a launch.  The caller keeps its pool of received bursts and only lists windows; there is no device state and
 * no handle.
 *
 * Limits.  NOT built: window jobs of the frame decoders (a call's frame array does not hold earlier calls' bursts), and so
 * no N = 4 / 8 inside tetra_rx / tetra_wbrx either, whose routing of the traffic slots the host names is N = 1 (tetra_traffic.h); speech
 * (TCH/S); an encoder.  TCH/7.2 is not coded and not interleaved: TETRA_ERR_ARG.
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_TCH_NBLK_H
#define TETRA_TCH_NBLK_H

#include <stdint.h>

#include "../tetra_lmac.h"
#include "tetra_tch.h"
#include "tetra_tch_soft.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Hard bits.
 *   kind          TETRA_LMAC_T_TCH_4_8 or TETRA_LMAC_T_TCH_2_4 (anything else: TETRA_ERR_ARG)
 *   n_interleave  1, 4 or 8 (anything else: TETRA_ERR_ARG)
 *   d_type5       [n_rows][in_stride] uint8, the caller's pool of received bursts, 432 bytes used per row (4-byte aligned, in_stride a
 *                 multiple of 4 and >= 432; n_rows >= 0)
 *   d_scramb_init the scrambling code of INPUT row r is d_scramb_init[d_init_index ? d_init_index[r] : r]
 *   d_windows     [n_blocks][n_interleave] int32 (4-byte aligned, not NULL): entry j of block b names the pool row that carries its j-th
 *                 diagonal.  Any entry outside [0, n_rows) means that burst is lost; -1 is the documented value, every other
 *                 out-of-range value behaves identically, and nothing is read for it.  Entries may repeat and need not slide.
 *   d_n_blocks    NULL, or the number of windows present, read on the device; blocks past it are not touched
 *   d_type2       [n_blocks][out_stride] uint8 out, type2 bytes per block (4-byte aligned, out_stride a multiple of 4 and >= type2); the
 *                 padding behind a row is not written
 *   d_biterr      NULL, or [n_blocks] uint32 out (4-byte aligned): the count defined above
 * Statuses as tetra_lmac_decode_tch_counted_device.  A workgroup (64 blocks) whose windows are complete and whose bytes are all 0 / 1
 * takes the decoder's packed route, any other its class route (tetra_lmac_debug_force_byte_route forces it); the results are the same
 * bit for bit.  n_blocks == 0 is a no-op.  Enqueued on hip_stream, no synchronisation; the decision scratch comes from the library's
 * stream-ordered pool.
 */
int tetra_lmac_decode_tch_nblk_device(int kind, int n_interleave, const uint8_t* d_type5, int n_rows, int in_stride,
                                      const uint32_t* d_scramb_init, const int32_t* d_init_index, const int32_t* d_windows, int n_blocks,
                                      const int32_t* d_n_blocks, uint8_t* d_type2, int out_stride, uint32_t* d_biterr, void* hip_stream);

/* Soft values: the same with d_soft [n_rows][in_stride] int8. */
int tetra_lmac_decode_tch_nblk_soft_device(int kind, int n_interleave, const int8_t* d_soft, int n_rows, int in_stride,
                                           const uint32_t* d_scramb_init, const int32_t* d_init_index, const int32_t* d_windows, int n_blocks,
                                           const int32_t* d_n_blocks, uint8_t* d_type2, int out_stride, uint32_t* d_biterr, void* hip_stream);

/*
 * Host-pointer variants (copy in/out, synchronise; device = HIP ordinal or -1 for the current one): scramb_init [n_rows] holds the code
 * of every pool row, biterr may be NULL.
 */
int tetra_lmac_decode_tch_nblk_batch(int kind, int n_interleave, const uint8_t* type5, int n_rows, int in_stride, const uint32_t* scramb_init,
                                     const int32_t* windows, int n_blocks, uint8_t* type2, int out_stride, uint32_t* biterr, int device);
int tetra_lmac_decode_tch_nblk_soft_batch(int kind, int n_interleave, const int8_t* soft5, int n_rows, int in_stride, const uint32_t* scramb_init,
                                          const int32_t* windows, int n_blocks, uint8_t* type2, int out_stride, uint32_t* biterr, int device);

#ifdef __cplusplus
}
#endif
#endif
