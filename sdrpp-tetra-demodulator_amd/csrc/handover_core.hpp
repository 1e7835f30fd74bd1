// handover_core.hpp -- lane code of the hand-over's two steps outside the synchroniser (include/ext/tetra_handover.h): the planting of
// an heir from its donor (tetra_retune.hip: k_handover_plant, behind the plain reset of the heir) and the apply step that carries the
// synchroniser's result word into the heir's cell (tetra_rx.hip: k_handover_apply, in front of the tracker).  The ASSIST state itself is
// bsync_core.hpp's.  Host- and device-callable (tests/emul/handover_emul.cpp runs it on the host); plain stores only; one lane per channel.
//
// A header of its own beside retune_core.hpp: it works on the synchroniser's State and Assist and on the tracker's state and clock step
// as bsync_core.hpp and lmac_core.hpp define them, and retune_core.hpp stays free of other stages' cores.
#pragma once

#include <cstdint>

#include "bsync_core.hpp"
#include "lmac_core.hpp"

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define HO_HD __host__ __device__ __forceinline__
#else
#define HO_HD inline
#endif

namespace handover {

// The channels' State, Assist and cell state (TrackState = tetra_lmac_cell_state_t member for member) where the stages keep them.
struct View {
    bsync_core::State* state;                 // [C] (not needed by the apply step)
    bsync_core::Assist* assist;               // [C]
    tetra_lmac::TrackState* cell;             // [C]
};

// expect = (F - B) + 510 m with the smallest m for which expect - W >= 0; F - B = -bits_in_buf
HO_HD int32_t plant_expect(uint32_t bits_in_buf, int32_t window, int32_t& m) {
    const int32_t need = (int32_t)bits_in_buf + window;                    // 510 m >= need
    m = need <= 0 ? 0 : (need + bsync_core::kTs - 1) / bsync_core::kTs;
    return bsync_core::kTs * m - (int32_t)bits_in_buf;
}
// k tetra_tdma_time_add_tn steps
HO_HD tetra_lmac::Tdma tdma_steps(tetra_lmac::Tdma t, int32_t k) {
    for (int32_t i = 0; i < k; ++i) tetra_lmac::tdma_add_tn(t);
    return t;
}
// The planting of heir c from `donor`, behind the plain reset of c (its State, bit buffer, cell and Assist all zero).  A donor that is
// not LOCKED or has no scrambling code: only the status is written.
HO_HD void plant_channel(const View& v, int c, int donor, int32_t window, int32_t max_slots) {
    const bsync_core::State d = v.state[donor];
    const tetra_lmac::TrackState dc = v.cell[donor];
    bsync_core::Assist as = { bsync_core::kHoRefused, 0, 0, 0u, 0, 0, 0, 0 };
    if (d.state == bsync_core::kLocked && dc.scramb_init != 0u) {
        int32_t m = 0;
        as.status = bsync_core::kHoPending;
        as.expect = (uint32_t)plant_expect(d.bits_in_buf, window, m);
        as.window = window;
        as.slots_left = max_slots;
        tetra_lmac::TrackState hc = dc;
        hc.phy = tdma_steps(dc.phy, m);
        v.cell[c] = hc;
        v.state[c].state = bsync_core::kAssist;
    }
    v.assist[c] = as;
}
// The synchroniser's result word of channel c, consumed: 1 + k advances the PHY time by k slots, -1 zeroes the cell.
HO_HD void apply_channel(const View& v, int c) {
    const int32_t r = v.assist[c].result;
    if (r == 0) return;
    v.assist[c].result = 0;
    if (r > 0) v.cell[c].phy = tdma_steps(v.cell[c].phy, r - 1);
    else v.cell[c] = tetra_lmac::TrackState{};
}

}  // namespace handover
