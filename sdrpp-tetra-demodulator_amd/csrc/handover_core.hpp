// handover_core.hpp -- lane code of the hand-over's two steps outside the synchroniser (include/ext/tetra_handover.h): the planting of
// an heir from its donor (tetra_retune.hip: k_handover_plant, behind the plain reset of the heir) and the apply step that carries the
// synchroniser's result word into the heir's cell (tetra_rx.hip: k_handover_apply, in front of the tracker), and of a stream gap
// (include/ext/tetra_gap.h; tetra_retune.hip: k_resume_tail), in which a channel is its own donor.  The ASSIST state itself is
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
// ---- stream gaps (include/ext/tetra_gap.h): a channel restarts as its own heir after `elapsed` bits that never arrived ----------------------
// The anchor of a channel: a frame at bit number a + 510 j is given the time q + j + 1 by the tracker; d = received bits - a.  LOCKED:
// a = bitbuf_start_bitnum, q = the PHY time; ASSIST with the status PENDING: a = expect, q = the PHY time advanced by the slot periods
// ASSIST has waited.  Anything else, or no scrambling code: not ok.  cell: the channel's cell with phy = q.
struct Anchor {
    int32_t ok;
    int32_t d;
    tetra_lmac::TrackState cell;
};
// the clock's period: 4 slots x 18 frames x 60 multiframes
constexpr int32_t kTdmaPeriod = 4320;
// Read before the channel is restarted.
HO_HD Anchor gap_anchor(const View& v, int c) {
    const bsync_core::State s = v.state[c];
    const bsync_core::Assist as = v.assist[c];
    Anchor an = { 0, 0, v.cell[c] };
    const uint32_t rcv = s.bitbuf_start_bitnum + s.bits_in_buf;
    if (an.cell.scramb_init == 0u) return an;
    if (s.state == bsync_core::kLocked) {
        an.ok = 1;
        an.d = (int32_t)(rcv - s.bitbuf_start_bitnum);
    } else if (s.state == bsync_core::kAssist && as.status == bsync_core::kHoPending) {
        an.ok = 1;
        an.d = (int32_t)(rcv - as.expect);
        an.cell.phy = tdma_steps(an.cell.phy, as.waited);
    }
    return an;
}
// expect = 510 m - (d + elapsed) with the smallest m >= 0 for which expect >= W; 0 <= elapsed <= 2^31 - 1.  With elapsed = 0 on a LOCKED
// channel (d = bits_in_buf) this is plant_expect.
HO_HD int32_t gap_expect(int32_t d, uint32_t elapsed, int32_t window, int32_t& m) {
    const long long need = (long long)d + (long long)elapsed + window;     // 510 m >= need
    const long long mm = need <= 0 ? 0 : (need + bsync_core::kTs - 1) / bsync_core::kTs;
    m = (int32_t)mm;
    return (int32_t)(bsync_core::kTs * mm - ((long long)d + (long long)elapsed));
}
// Channel c behind its plain reset (State, bit buffer, cell and Assist all zero), from its own anchor: ASSIST around the frame start the
// anchor's grid gives after the gap, the clock advanced by the slots that passed (m mod the clock's period steps: the same time).
HO_HD void resume_channel(const View& v, int c, const Anchor& an, uint32_t elapsed, int32_t window, int32_t max_slots) {
    bsync_core::Assist as = { bsync_core::kHoRefused, 0, 0, 0u, 0, 0, 0, 0 };
    if (an.ok) {
        int32_t m = 0;
        as.status = bsync_core::kHoPending;
        as.expect = (uint32_t)gap_expect(an.d, elapsed, window, m);
        as.window = window;
        as.slots_left = max_slots;
        tetra_lmac::TrackState hc = an.cell;
        hc.phy = tdma_steps(an.cell.phy, m % kTdmaPeriod);
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
