// Host build of the stream gap's lane code (include/ext/tetra_gap.h): the anchor, the planting arithmetic and the resume of a channel as
// its own heir (sdrpp-tetra-demodulator_amd/csrc/handover_core.hpp) around the plain reset of the channel (csrc/retune_core.hpp), in the
// order of tetra_retune.hip's k_resume_tail with its 64 lanes done one after the other.  The ASSIST state that a resumed channel runs in
// is handover_emul.cpp's.  TEST TOOL.
#define TETRA_HOST_EMUL 1
#include <cstdint>

#include "../../sdrpp-tetra-demodulator_amd/csrc/handover_core.hpp"
#include "../../sdrpp-tetra-demodulator_amd/csrc/retune_core.hpp"

using namespace bsync_core;

extern "C" {

int gap_emul_tdma_period(void) { return handover::kTdmaPeriod; }

// expect and m of the rule for the anchor distance d = Rcv - a and G elapsed bits
int gap_emul_expect(int32_t d, uint32_t elapsed, int window, int32_t* m) { return handover::gap_expect(d, elapsed, window, *m); }

// the anchor of channel c: returns ok, *d = Rcv - a, q = {tn, fn, mn}
int gap_emul_anchor(State* states, Assist* assist, tetra_lmac::TrackState* cell, int c, int32_t* d, uint32_t* q) {
    const handover::Anchor an = handover::gap_anchor(handover::View{ states, assist, cell }, c);
    *d = an.d;
    q[0] = an.cell.phy.tn; q[1] = an.cell.phy.fn; q[2] = an.cell.phy.mn;
    return an.ok;
}

// states [C][4 words], assist [C][8], cell [C][10], carry [C][4096 bytes], miss [C]: channel c resumes after `elapsed` bits
void gap_emul_resume(State* states, Assist* assist, tetra_lmac::TrackState* cell, uint8_t* carry, int32_t* miss, int c, uint32_t elapsed, int window,
                     int max_slots) {
    constexpr int kLanes = 64;
    const handover::View v = { states, assist, cell };
    const retune::BsyncView b = { reinterpret_cast<uint32_t*>(states), reinterpret_cast<uint32_t*>(carry), (int32_t)(sizeof(State) / 4), kBuf / 4 };
    const retune::CellView cv = { reinterpret_cast<uint32_t*>(cell), (int32_t)(sizeof(tetra_lmac::TrackState) / 4) };
    const retune::CellView mv = { reinterpret_cast<uint32_t*>(miss), 1 };
    const retune::CellView av = { reinterpret_cast<uint32_t*>(assist), kAssistWords };
    const handover::Anchor an = handover::gap_anchor(v, c);
    for (int lane = 0; lane < kLanes; ++lane) {
        retune::reset_bsync_channel(b, c, lane, kLanes);
        retune::reset_cell_channel(cv, c, lane, kLanes);
        retune::reset_cell_channel(mv, c, lane, kLanes);
        retune::reset_cell_channel(av, c, lane, kLanes);
    }
    handover::resume_channel(v, c, an, elapsed, window, max_slots);
}

}  // extern "C"
