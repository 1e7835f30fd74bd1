// rx_snap_impl.hpp -- what the receive chain's per-call snapshot (include/ext/tetra_rx_out_ext.h) needs from the synchroniser, whose
// handle is private to tetra_burst_sync.hip: its per-channel tables where they are.  Host-side, hidden from the C ABI.
#pragma once

#include "../../include/tetra_burst_sync.h"

namespace rx_snap_impl {

// *state [n_channels]; *miss [n_channels] int32, null until the handle was first switched to the tolerant rule (ext/tetra_sync_tol.h)
__attribute__((visibility("hidden"))) int bsync_tables(tetra_bsync_t* h, const tetra_bsync_state_t** state, const int32_t** miss);

}  // namespace rx_snap_impl
