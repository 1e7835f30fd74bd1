// lmac_impl.hpp -- what the receive chain (tetra_rx.hip) needs from the frame decoder (tetra_lmac.hip) beyond include/tetra_lmac.h:
// the soft-decision launch behind TETRA_RX_FLAG_SOFT.  Host-side, hidden from the C ABI.
#pragma once

#include <stdint.h>

#include "../../include/tetra_lmac.h"

#ifndef TETRA_HIDDEN
#define TETRA_HIDDEN __attribute__((visibility("hidden")))
#endif

namespace lmac_impl {

// the chain's soft values (soft_core.hpp): one int8 per bit, [n_channels][size], a channel's bit n at n mod size (a power of two);
// channel = frame slot / frames_per_channel of the frame source
struct SoftRing {
    const int8_t* d_ring;
    uint32_t size;
};

// Where the list launches (tetra_list.h) keep the compacted failed rows: list_work_bytes(jobs) bytes of device memory, 4-byte aligned,
// for one launch at a time; d_work = NULL: leased from the decoder's keeping pool per launch.
struct ListWork {
    void* d_work = nullptr;
    size_t bytes = 0;
};
TETRA_HIDDEN size_t list_work_bytes(const tetra_lmac_job_t* jobs, int n_jobs);

// tetra_lmac_decode_frames_device for the coded kinds (SB1, SB2, NDB, SCH/F; a BBK job is TETRA_ERR_ARG: the AACH stays on the packed
// frames), the block's bits read as soft values from the ring at the frame's bit number (src->d_frame_bitnum, required) and
// src->frames_per_channel >= 1.  Same jobs, rows, verdicts, labels and workspace as the entry point it mirrors.  d_biterr: as
// tetra_lmac_decode_frames_biterr_device's (tetra_biterr.h), the counts taken on the soft values.  max_candidates, d_rank: as
// tetra_lmac_decode_frames_list_device's (tetra_list.h), the margins taken on the soft values.
TETRA_HIDDEN int decode_frames_soft(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, const SoftRing& ring, void* hip_stream,
                                    uint32_t* const* d_biterr = nullptr, int max_candidates = 0, int32_t* const* d_rank = nullptr,
                                    ListWork list_work = ListWork());

// tetra_lmac_decode_frames_biterr_device and tetra_lmac_decode_frames_list_device in one: counts and ranks per job, either array may be
// NULL (the chain with TETRA_RX_FLAG_LIST, with or without TETRA_RX_FLAG_BITERR).
TETRA_HIDDEN int decode_frames_list(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, void* hip_stream, uint32_t* const* d_biterr,
                                    int max_candidates, int32_t* const* d_rank, ListWork list_work = ListWork());

}  // namespace lmac_impl
