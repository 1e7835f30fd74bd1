// lmac_impl.hpp -- the frame decoder (tetra_lmac.hip) as its callers inside the library see it: ONE function, decode_frames, that takes
// every option of a frame launch as a FrameOpts.  The frame entry points of the C ABI (tetra_lmac_decode_frames_device,
// _biterr_device, _list_device, _soft_device, _soft_tch_device) are it with the options their signatures can express; the receive chain (tetra_rx.hip) builds the
// options from its handle's flags -- soft values from the chain's ring, bit-error counts, ranks, where the list launches keep their work --
// and calls it directly.  Host-side, hidden from the C ABI.
#pragma once

#include <stddef.h>
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

// The options of a frame launch; the defaults are tetra_lmac_decode_frames_device.
struct FrameOpts {
    // NULL: the blocks' bits from the packed frames.  Else the coded kinds (SB1, SB2, NDB, SCH/F; a BBK job is TETRA_ERR_ARG unless it
    // carries TETRA_LMAC_JOB_RM3014_SOFT, tetra_aach_soft.h: the AACH by maximum likelihood, launches of its own behind the decode launch) read as soft values from this ring at the frame's bit number: a ring of whole aligned words, and
    // src->d_frame_bitnum and src->frames_per_channel >= 1 are required.  Counts and margins are then taken on the soft values.
    const SoftRing* soft = nullptr;
    uint32_t* const* d_biterr = nullptr;        // NULL, or per job where its counts go (NULL: the job does not count), tetra_biterr.h
    int32_t* const* d_rank = nullptr;           // NULL, or per job where its ranks go (NULL: the job is not rescued), tetra_list.h
    int max_candidates = 0;                     // the ranks' T; looked at only for a job with ranks
    ListWork list_work;
    bool soft_tch = false;                      // with soft: TCH/4.8 and TCH/2.4 jobs are accepted and read the ring too (tetra_tch_soft.h)
};

// tetra_lmac_decode_frames_device with options: same jobs, rows, verdicts, labels and workspace.  Launches on the stream: the decode
// kernel, the list launches if any job has ranks, the hand-back of the decision scratch.
TETRA_HIDDEN int decode_frames(const tetra_lmac_frames_t* src, const tetra_lmac_job_t* jobs, int n_jobs, const FrameOpts& opts, void* hip_stream);

}  // namespace lmac_impl
