// retune_impl.hpp -- what tetra_retune.hip and the receive chain (rx_handle.hpp) need from the stages whose handles are private to
// their sources: views of their per-channel state (retune_core.hpp), the synchroniser's per-channel tables where they are, and the
// resampler's switch to picked columns.  Host-side, hidden from the C ABI.
#pragma once

#include "../../include/tetra_burst_sync.h"
#include "../../include/tetra_chan.h"
#include "../../include/tetra_demod.h"
#include "retune_core.hpp"

#define TETRA_HIDDEN __attribute__((visibility("hidden")))

namespace retune_impl {

// tetra_demod.hip: the state arrays a reset of one channel writes, and `fresh` as tetra_demod_reset decides it under the handle's flags
TETRA_HIDDEN int demod_view(tetra_demod_t* h, retune::DemodView* out);
// tetra_burst_sync.hip
TETRA_HIDDEN int bsync_view(tetra_bsync_t* h, retune::BsyncView* out);
// ... and its per-channel tables on the device, [n_channels] each.  The miss counters exist from the first switch to the tolerant rule
// (ext/tetra_sync_tol.h) on and stay when the handle returns to the reference's rule: `miss` says whether they exist, `tolerant`
// whether they count.
// `assist`: the hand-over's fields (bsync_core::Assist; ext/tetra_handover.h), null until the handle's first hand-over.
struct BsyncTables {
    tetra_bsync_state_t* state;
    int32_t* miss;
    bool tolerant;
    void* assist;
};
TETRA_HIDDEN int bsync_tables(tetra_bsync_t* h, BsyncTables* out);
// ... the hand-over's fields, allocated and zeroed on the first call (which waits for the device, once); from then on the handle
// launches its ASSIST-capable kernels
TETRA_HIDDEN int bsync_assist(tetra_bsync_t* h, void** out);
// tetra_chan.hip: what tetra_chan_reset leaves -- delay line and carry cleared, the shift's phase reference at the next sample --,
// enqueued on `stream` (the one the process calls use) with no host synchronisation (ext/tetra_gap.h)
TETRA_HIDDEN int chan_restart(tetra_chan_t* h, void* stream);
// tetra_resamp.hip: a handle that runs all its channels in place (16-byte lane units) becomes one that picks columns (8-byte units,
// what TETRA_RESAMP_FLAG_NARROW_UNITS gives at create).  Same floats; the delay line's layout does not depend on the unit width.
TETRA_HIDDEN int resamp_narrow_units(tetra_resamp_t* h);

}  // namespace retune_impl
