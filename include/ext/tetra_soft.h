/*
 * tetra_soft.h -- C ABI of the frame decoder's soft-decision source: the coded kinds (SB1, SB2, NDB, SCH/F) decoded from soft values in a
 * ring instead of the packed frames' hard bits.
 *
 * The receive chain (tetra_rx.h, TETRA_RX_FLAG_SOFT) quantises the demodulator's symbols into one signed byte per bit, keeps them in a
 * ring per channel and hands that ring to the frame decoder.  The entry point declared here is the same launch for a caller that has
 * soft values of its own: the frames say WHERE a block lies (burst type, bit number, channel), the ring holds WHAT was received there.
 * The decoder is the reference's conv_cch_decode on those values -- descrambled by sign, deinterleaved, depunctured onto zeros -- bit
 * for bit, with the CRC verdict on top; the receive chain keeps calling the decoder directly, nothing about it changes.
 * Limits.  The circuit-mode data channels (tetra_tch.h) are not among the kinds of this entry point: a TCH job is TETRA_ERR_ARG here.
 * tetra_tch_soft.h declares the entry that takes TCH/4.8 and TCH/2.4 jobs beside these kinds, and the int8 byte-row entries.
 * Same conventions as tetra_lmac.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_SOFT_H
#define TETRA_SOFT_H

#include <stdint.h>

#include "../tetra_lmac.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * tetra_lmac_decode_frames_device on soft values: src, jobs and n_jobs as there (rows, verdicts, labels, device-side row counts, the
 * workspace), and statuses as there, plus
 *   d_ring          [ceil(src->n_frames / src->frames_per_channel)][ring_size] int8 on the device, one soft value per bit, 4-byte
 *                   aligned.  Channel c = frame / frames_per_channel owns row c; its bit number n sits at n mod ring_size.  Positive
 *                   means bit 0, negative bit 1, zero carries no decision (an erasure); |value| <= 31 (six bits: the bound under
 *                   which the decoder's packed 16-bit path metrics need no renormalisation).  Values outside are not checked for.
 *   ring_size       a power of two >= 4; a frame's 510 bits may wrap the ring's end, and bit numbers wrap at 2^32 as the ring does.
 *                   A ring shorter than a burst (512) cannot hold a frame's bits side by side.
 *   src             d_frame_bitnum [n_frames] is REQUIRED (the absolute bit number of each frame's first bit) and
 *                   frames_per_channel >= 1, with or without labels.  d_frames is not read for the coded kinds, but must be given and
 *                   aligned as for tetra_lmac_decode_frames_device; d_frame_type says which kinds a frame carries.
 *   jobs            SB1, SB2, NDB and SCH/F.  A BBK job (with or without TETRA_LMAC_JOB_RM3014) is TETRA_ERR_ARG: the AACH's hard bits are
 *                   not in the ring, decode them from the packed frames.  The AACH's soft route is a job flag of its own,
 *                   TETRA_LMAC_JOB_RM3014_SOFT of ext/tetra_aach_soft.h, which this entry point alone accepts.  A listed frame of another burst type decodes as a block of erasures
 *                   (all soft values zero) under that frame's scrambling code.
 *   d_biterr        NULL, or [n_jobs] device pointers as for tetra_lmac_decode_frames_biterr_device (tetra_biterr.h); an entry may be
 *                   NULL.  The counts are taken on the soft values: compared = the positions whose value is not 0, errors = those
 *                   whose sign differs from the re-encoded block.
 *   d_rank          NULL, or [n_jobs] device pointers as for tetra_lmac_decode_frames_list_device (tetra_list.h); an entry may be
 *                   NULL.  The margins are in raw soft units, and the rescue stages its rows from the ring again: d_ring must stay
 *                   valid and unchanged until the call's work on the stream is done.  With counts, a rescued row's count is that of
 *                   the rescued codeword.
 *   max_candidates  the ranks' T, 1..TETRA_LIST_MAX_CANDIDATES (else TETRA_ERR_ARG for a job with ranks); not looked at otherwise.
 * TETRA_ERR_ARG, before anything is launched or written: d_ring NULL or off the 4-byte grid, ring_size 0 / below 4 / no power of two,
 * src->d_frame_bitnum NULL, src->frames_per_channel < 1, a BBK job without TETRA_LMAC_JOB_RM3014_SOFT.
 */
int tetra_lmac_decode_frames_soft_device(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs,
                                         const int8_t* d_ring, uint32_t ring_size,
                                         uint32_t* const* d_biterr, int32_t* const* d_rank, int max_candidates,
                                         void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
