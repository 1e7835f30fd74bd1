/*
 * tetra_aach.h -- C ABI of the AACH's channel decoding: the shortened (30,14) Reed-Muller code of EN 300 392-2 8.2.3.2, decoded on
 * the device with error correction.
 *
 * The AACH (access-assignment channel, TPSAP_T_BBK) is in every downlink burst and is the one block the reference delivers without
 * channel decoding: tp_sap_udata_ind only descrambles it and reports crc_ok = 1 (src/decoder/src/lower_mac/tetra_lower_mac.c:230-236,
 * "FIXME: RM3014-decode"; lower_mac/tetra_rm3014.c:88-96 has the encoder and a decoder stub).  By default this library does the same
 * (tetra_lmac.h, tetra_rx.h).  The entry points and options declared here are OPT-IN and change nothing unless used.
 *
 * The code has minimum distance 8, so a word with up to 3 bit errors has exactly one codeword within distance 3 and every word with
 * 4 errors has none.  Decoding is bounded-distance with radius 3:
 *     a codeword within Hamming distance <= 3 of the received word   ->  that codeword, dist = the distance (0..3), crc_ok = 1
 *     none                                                           ->  the received word unchanged, dist = 0xFF,  crc_ok = 0
 * crc_ok = 0 for an AACH DEPARTS FROM THE REFERENCE, which always reports 1; it is what lets a consumer tell a damaged AACH from a
 * clean one.  A lane decodes with one syndrome (14 AND / XOR steps) and one look-up in a table syndrome -> error pattern (2^16
 * entries, 256 KB) that the library builds on the host from the generator matrix on first use, once per device, and keeps with its
 * other per-device constants (the scrambling-sequence table, the scratch pool) for the life of the process.
 *
 * Word format: the block's 30 bits, first bit on air at bit 29 -- information bits in bits 29..16, parity bits in bits 15..0, the
 * value format of the reference's tetra_rm3014_compute.  Row format with the option on (32 bytes per row):
 *     bytes 0..29   one bit per byte: the corrected codeword (dist <= 3), else the descrambled bits as without the option
 *     byte 30       dist (0..3, or 0xFF)
 *     byte 31       0
 * The first 14 bytes are the type-1 bits (the ACCESS-ASSIGN PDU; parsing it is upper MAC and stays with the caller).
 * Decoding the same code from SOFT values, by exact maximum likelihood over its 16384 codewords, is ext/tetra_aach_soft.h
 * (TETRA_LMAC_JOB_RM3014_SOFT, TETRA_RX_FLAG_AACH_SOFT): an option of its own that excludes the ones declared here.
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_AACH_H
#define TETRA_AACH_H

#include <stdint.h>

#include "tetra_lmac.h"
#include "tetra_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TETRA_AACH_UNDECODABLE 0xFF

/*
 * The bare primitive on n 30-bit words (bits 31..30 of an input word are ignored):
 *   d_words      [n] uint32 in
 *   d_out_words  [n] uint32 out: the codeword, or the input word (30 bits) where dist = 0xFF; may equal d_words
 *   d_dist       [n] uint8 out
 * Enqueued on hip_stream of the current device, no synchronisation.  n == 0 is a no-op.
 */
int tetra_lmac_rm3014_decode_device(const uint32_t* d_words, int n, uint32_t* d_out_words, uint8_t* d_dist, void* hip_stream);

/*
 * Byte rows: tetra_lmac_decode_batch_device for TETRA_TPSAP_T_BBK, with the Reed-Muller decoding behind the descrambler.
 *   d_type5        [n_blocks][in_stride] uint8, one bit per byte, 30 used (4-byte aligned, in_stride a multiple of 4 and >= 30)
 *   d_scramb_init  [n_blocks] uint32
 *   d_type2        [n_blocks][out_stride] uint8 out: rows as above (4-byte aligned, out_stride a multiple of 4 and >= 32)
 *   d_crc_ok       [n_blocks] int32 out: 1 where dist <= 3, else 0
 * The decoder's input is the 30 descrambled bytes the pass-through writes, a byte other than 0 counting as a 1 (erasures are not
 * used: hard decision).  AACH rows have one route through the decoder; tetra_lmac_debug_force_byte_route does not change it.
 */
int tetra_lmac_decode_aach_rm3014_device(const uint8_t* d_type5, int n_blocks, int in_stride, const uint32_t* d_scramb_init,
                                         uint8_t* d_type2, int out_stride, int32_t* d_crc_ok, void* hip_stream);

/*
 * Decoding straight from packed frames (tetra_lmac_decode_frames_device): OR this into tetra_lmac_job_t.type of a TETRA_TPSAP_T_BBK
 * job and its rows, d_crc_ok and the labels' crc_ok follow the table above.  On any other type it is TETRA_ERR_ARG.  Every other
 * job of the launch is decoded exactly as without it.
 */
#define TETRA_LMAC_JOB_RM3014 0x100

/*
 * The receive chain: TETRA_RX_FLAG_AACH_RM3014 in tetra_rx_config_t.flags (tetra_rx.h; through cfg.rx also for tetra_wbrx_create)
 * makes the chain's BBK job decode with the code.  tetra_rx_fetch(TETRA_RX_KIND_BBK) then returns the 30 corrected bits and the
 * verdict in crc_ok, tetra_rx_rows_device the rows as above, and the tetra_rx_out.h delivery with TETRA_RX_OUT_CRC_GOOD keeps only
 * the decodable AACH rows.  A delivery carries the 30 bits; the distance (byte 30) comes with them as a column of an extended
 * delivery (ext/tetra_rx_out_ext.h, TETRA_RX_OUT_EXT_ROW_AACH_DIST), or through the blocking fetch below.
 *
 * tetra_rx_fetch_aach_dist: byte 30 of every BBK row of the latest (which = 0) or previous (1) call, in tetra_rx_fetch's order.
 *   dist     [capacity] uint8 host, may be NULL
 *   *n_rows  rows available; more than capacity with dist != NULL: TETRA_ERR_SIZE and nothing is copied
 * TETRA_ERR_UNSUPPORTED if the handle was created without the flag or does not decode BBK.  Before the first call / which = 1 before
 * the second: 0 rows.
 */
int tetra_rx_fetch_aach_dist(tetra_rx_t* h, int which, uint8_t* dist, int capacity, int* n_rows);

#ifdef __cplusplus
}
#endif
#endif
