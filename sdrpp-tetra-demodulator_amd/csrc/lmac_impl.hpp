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

// tetra_lmac_decode_frames_device for the coded kinds (SB1, SB2, NDB, SCH/F; a BBK job is TETRA_ERR_ARG: the AACH stays on the packed
// frames), the block's bits read as soft values from the ring at the frame's bit number (src->d_frame_bitnum, required) and
// src->frames_per_channel >= 1.  Same jobs, rows, verdicts, labels and workspace as the entry point it mirrors.  d_biterr: as
// tetra_lmac_decode_frames_biterr_device's (tetra_biterr.h), the counts taken on the soft values.
TETRA_HIDDEN int decode_frames_soft(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, const SoftRing& ring, void* hip_stream,
                                    uint32_t* const* d_biterr = nullptr);

}  // namespace lmac_impl
