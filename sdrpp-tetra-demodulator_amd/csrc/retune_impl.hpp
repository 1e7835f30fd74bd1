// retune_impl.hpp -- what tetra_retune.hip needs from the stages whose handles are private to their sources: views of their
// per-channel state (retune_core.hpp) and the resampler's switch to picked columns.  Host-side, hidden from the C ABI.
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
TETRA_HIDDEN int bsync_miss_view(tetra_bsync_t* h, retune::CellView* out);
// tetra_resamp.hip: a handle that runs all its channels in place (16-byte lane units) becomes one that picks columns (8-byte units,
// what TETRA_RESAMP_FLAG_NARROW_UNITS gives at create).  Same floats; the delay line's layout does not depend on the unit width.
TETRA_HIDDEN int resamp_narrow_units(tetra_resamp_t* h);

}  // namespace retune_impl
