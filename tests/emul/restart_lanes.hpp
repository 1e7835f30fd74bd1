// The tail part of a channel's restart on the host, in the order of tetra_retune.hip's k_restart_tail with its lanes done one after the
// other: the source's anchor (csrc/handover_core.hpp), the clearing of every tail table (csrc/retune_core.hpp: reset_tail_channel), the
// planting.  What the host emulations of the reset, the hand-over and the stream gap share.  TEST TOOL.
#pragma once
#define TETRA_HOST_EMUL 1
#include <cstdint>

#include "../../sdrpp-tetra-demodulator_amd/csrc/handover_core.hpp"

namespace restart_emul {

// states [C][4 words], carry [C][4096 bytes], cell [C][10], link [C][link_words], miss [C], assist [C][8]; carry, link, miss and assist may
// be null: a table that is not kept
inline retune::TailView tail_view(bsync_core::State* states, uint8_t* carry, tetra_lmac::TrackState* cell, uint32_t* link, int link_words, int32_t* miss,
                                  bsync_core::Assist* assist) {
    return { { reinterpret_cast<uint32_t*>(states), reinterpret_cast<uint32_t*>(carry), (int32_t)(sizeof(bsync_core::State) / 4), carry ? bsync_core::kBuf / 4 : 0 },
             { reinterpret_cast<uint32_t*>(cell), (int32_t)(sizeof(tetra_lmac::TrackState) / 4) },
             { link, link ? link_words : 0 },
             { reinterpret_cast<uint32_t*>(miss), miss ? 1 : 0 },
             { reinterpret_cast<uint32_t*>(assist), assist ? bsync_core::kAssistWords : 0 } };
}

// src < 0: a plain reset.  Else c is planted from src's anchor: a donor (accept_pending = 0, elapsed = 0) or c itself after a gap (1).
inline void restart_channel(const retune::TailView& t, int c, int src, int accept_pending, uint32_t elapsed, int window, int max_slots, int lanes = 64) {
    const handover::View v = handover::view_of(t);
    handover::Anchor an = {};
    if (src >= 0) an = handover::anchor_of(v, src, accept_pending != 0);
    for (int lane = lanes - 1; lane >= 0; --lane) retune::reset_tail_channel(t, c, lane, lanes);
    if (src >= 0) handover::plant(v, c, an, elapsed, window, max_slots);
}

}  // namespace restart_emul
