// handover_core.hpp -- lane code of a restart that keeps frame timing, cell and clock: the hand-over (include/ext/tetra_handover.h), in
// which an heir is planted from its donor, and the stream gap (include/ext/tetra_gap.h), a hand-over in which every channel is its own
// donor and a known time has passed.  Both are the source's anchor read before the plain reset of the channel (retune_core.hpp:
// reset_tail_channel) and one planting behind it (tetra_retune.hip: k_restart_tail); the apply step carries the synchroniser's result
// word into the heir's cell (tetra_rx.hip: k_handover_apply, in front of the tracker).  The ASSIST state itself is bsync_core.hpp's.
// Host- and device-callable (tests/emul/restart_lanes.hpp runs it on the host); plain stores only; one lane per channel.
//
// A header of its own beside retune_core.hpp: it works on the synchroniser's State and Assist and on the tracker's state and clock step
// as bsync_core.hpp and lmac_core.hpp define them, and retune_core.hpp stays free of other stages' cores.
#pragma once

#include <cstdint>

#include "bsync_core.hpp"
#include "lmac_core.hpp"
#include "retune_core.hpp"

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
// ... as the tail's tables hold them
HO_HD View view_of(const retune::TailView& t) {
    return { reinterpret_cast<bsync_core::State*>(t.sync.state), reinterpret_cast<bsync_core::Assist*>(t.assist.cell),
             reinterpret_cast<tetra_lmac::TrackState*>(t.cell.cell) };
}

// the clock's period: 4 slots x 18 frames x 60 multiframes
constexpr int32_t kTdmaPeriod = 4320;

// k tetra_tdma_time_add_tn steps
HO_HD tetra_lmac::Tdma tdma_steps(tetra_lmac::Tdma t, int32_t k) {
    for (int32_t i = 0; i < k; ++i) tetra_lmac::tdma_add_tn(t);
    return t;
}
// The anchor of a channel: a frame at bit number a + 510 j is given the time q + j + 1 by the tracker; d = received bits - a.  LOCKED:
// a = bitbuf_start_bitnum (d = bits_in_buf), q = the PHY time; with accept_pending also ASSIST with the status PENDING: a = expect, q = the
// PHY time advanced by the slot periods ASSIST has waited.  Anything else, or no scrambling code: not ok.  cell: the channel's cell with
// phy = q.
struct Anchor {
    int32_t ok;
    int32_t d;
    tetra_lmac::TrackState cell;
};
// Read before anything is restarted.  A donor must be LOCKED (accept_pending = false); a channel that is its own source may be PENDING.
HO_HD Anchor anchor_of(const View& v, int src, bool accept_pending) {
    const bsync_core::State s = v.state[src];
    Anchor an = { 0, 0, v.cell[src] };
    if (an.cell.scramb_init == 0u) return an;
    if (s.state == bsync_core::kLocked) {
        an.ok = 1;
        an.d = (int32_t)s.bits_in_buf;
    } else if (accept_pending && s.state == bsync_core::kAssist && v.assist[src].status == bsync_core::kHoPending) {
        const bsync_core::Assist as = v.assist[src];
        an.ok = 1;
        an.d = (int32_t)(s.bitbuf_start_bitnum + s.bits_in_buf - as.expect);
        an.cell.phy = tdma_steps(an.cell.phy, as.waited);
    }
    return an;
}
// expect = 510 m - (d + elapsed) with the smallest m >= 0 for which expect >= W; 0 <= elapsed <= 2^31 - 1.  (A hand-over: elapsed = 0 and
// d = the donor's bits_in_buf, so expect = (F - B) + 510 m.)
HO_HD int32_t expect(int32_t d, uint32_t elapsed, int32_t window, int32_t& m) {
    const long long need = (long long)d + (long long)elapsed + window;     // 510 m >= need
    const long long mm = need <= 0 ? 0 : (need + bsync_core::kTs - 1) / bsync_core::kTs;
    m = (int32_t)mm;
    return (int32_t)(bsync_core::kTs * mm - ((long long)d + (long long)elapsed));
}
// Channel c behind its plain reset (State, bit buffer, cell and Assist all zero), from the anchor of its source: ASSIST around the frame
// start the anchor's grid gives `elapsed` bits on, the clock advanced by the slots that passed (m mod the clock's period steps: the same
// time).  An anchor that is not ok: only the status is written.
HO_HD void plant(const View& v, int c, const Anchor& an, uint32_t elapsed, int32_t window, int32_t max_slots) {
    bsync_core::Assist as = { bsync_core::kHoRefused, 0, 0, 0u, 0, 0, 0, 0 };
    if (an.ok) {
        int32_t m = 0;
        as.status = bsync_core::kHoPending;
        as.expect = (uint32_t)expect(an.d, elapsed, window, m);
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

// The names the hand-over's and the gap's lane code had while they were two: each is one call of the three functions above, kept so
// that a host build written against them (an emulation of an earlier commit) still compiles and runs this lane code.  Nothing in this
// tree calls them.
HO_HD int32_t plant_expect(uint32_t bits_in_buf, int32_t window, int32_t& m) { return expect((int32_t)bits_in_buf, 0u, window, m); }
HO_HD void plant_channel(const View& v, int c, int donor, int32_t window, int32_t max_slots) { plant(v, c, anchor_of(v, donor, false), 0u, window, max_slots); }
HO_HD Anchor gap_anchor(const View& v, int c) { return anchor_of(v, c, true); }
HO_HD int32_t gap_expect(int32_t d, uint32_t elapsed, int32_t window, int32_t& m) { return expect(d, elapsed, window, m); }
HO_HD void resume_channel(const View& v, int c, const Anchor& an, uint32_t elapsed, int32_t window, int32_t max_slots) { plant(v, c, an, elapsed, window, max_slots); }

}  // namespace handover
