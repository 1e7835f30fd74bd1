// Host build of the hand-over's lane code (include/ext/tetra_handover.h): the ASSIST state of the burst synchroniser's walk under both
// lock rules (sdrpp-tetra-demodulator_amd/csrc/bsync_core.hpp: AssistLock around RefLock / TolLock), and the planting and apply steps
// (csrc/handover_core.hpp) around the restart of a channel (restart_lanes.hpp), with the kernels' parallel phases done sequentially as in
// bsync_emul.cpp / bsync_tol_emul.cpp.  TEST TOOL.
#define TETRA_HOST_EMUL 1
#include <cstdint>
#include <cstring>
#include <vector>

#include "bsync_lane_io.hpp"
#include "restart_lanes.hpp"

using namespace bsync_core;

namespace {
// tol3 == null: the reference's lock rule; else {tol_norm, tol_sync, max_miss} and the channel's miss counter
int process(State* st, Assist* as, int32_t* misses, uint8_t* carry, const uint8_t* bits, int n_new, const int32_t* tol3, void* frames, int packed,
            int32_t* types, uint32_t* bitnums, int max_frames, int use_batch) {
    bsync_emul::Call call(*st, carry, bits, n_new, n_new, max_frames);
    const int words = (int)call.s.size(), x0 = kOff - (int)st->bits_in_buf, xe = kOff + n_new;
    const uint32_t* s = call.s.data();
    std::vector<uint32_t> ms(words, 0), m1(words, 0), m2(words, 0), ma(words, 0);
    for (int w = x0 >> 5; w <= (xe - 1) >> 5 && w + 2 < words; ++w) { match_word(s, w, x0, xe, ms[w], m1[w], m2[w]); ma[w] = ms[w] | m1[w] | m2[w]; }
    if (!tol3) {
        auto batch = [&](int bx, int K, int f0, uint32_t abs_bx, bool& unlocked) {
            if (!use_batch) return 0;
            int done = 0;
            while (done < K) {
                const FrameEval e = locked_frame_eval(s, ms.data(), m1.data(), m2.data(), ma.data(), bx + kTs * done);
                call.emit(f0 + done, bx + kTs * done, e.reported, abs_bx + (uint32_t)(kTs * done));
                done++;
                if (e.unlocks) { unlocked = true; break; }
            }
            return done;
        };
        RefLock inner{ ms.data(), m1.data(), m2.data(), ma.data() };
        AssistLock<RefLock> lock{ inner, *as };
        return call.finish([&](int& carry_x, auto first, auto emit) { return walk(*st, s, ms.data(), n_new, carry_x, first, emit, batch, lock); },
                           packed, carry, frames, types, bitnums);
    }
    const Tolerance tol = { tol3[0], tol3[1], tol3[2] };
    if (!tolerance_valid(tol)) return -2;
    int m = *misses;
    TolLock inner{ tol, m };
    auto batch = [&](int bx, int K, int f0, uint32_t abs_bx, bool& unlocked) {      // a round of 64 frames and the kernel's bit form of the miss rule
        if (!use_batch) return 0;
        int done = 0;
        while (done < K) {
            const int here = K - done < 64 ? K - done : 64;
            int reported[64];
            uint64_t pass = 0;
            for (int lane = 0; lane < 64; ++lane) {
                reported[lane] = lane < here ? tolerant_frame_eval(s, bx + kTs * (done + lane), tol) : -1;
                if (reported[lane] >= 0) pass |= 1ull << lane;
            }
            const Unlock u = first_unlock_bits(pass, here, m, tol.max_miss);
            const int take = u.index >= 0 ? u.index + 1 : here;
            for (int lane = 0; lane < take; ++lane) call.emit(f0 + done + lane, bx + kTs * (done + lane), reported[lane], abs_bx + (uint32_t)(kTs * (done + lane)));
            m = u.misses;
            done += take;
            if (u.index >= 0) { unlocked = true; break; }
        }
        return done;
    };
    AssistLock<TolLock> lock{ inner, *as };
    const int n = call.finish([&](int& carry_x, auto first, auto emit) { return walk(*st, s, ms.data(), n_new, carry_x, first, emit, batch, lock); },
                              packed, carry, frames, types, bitnums);
    *misses = m;
    return n;
}
}  // namespace

extern "C" {

int handover_emul_assist_words(void) { return kAssistWords; }

// one channel's call; frames [max_frames][512] bytes or, packed, [max_frames][16] words.  Returns the frame count, -1 on overflow.
int handover_emul_process(State* st, Assist* as, int32_t* misses, uint8_t* carry, const uint8_t* bits, int n_new, const int32_t* tol3, void* frames,
                          int packed, int32_t* types, uint32_t* bitnums, int max_frames, int use_batch) {
    return process(st, as, misses, carry, bits, n_new, tol3, frames, packed, types, bitnums, max_frames, use_batch);
}

// expect and m of the planting for a donor with bits_in_buf buffered bits
int handover_emul_expect(uint32_t bits_in_buf, int window, int32_t* m) { return handover::expect((int32_t)bits_in_buf, 0u, window, *m); }

// k tetra_tdma_time_add_tn steps on t = {tn, fn, mn}, in place
void handover_emul_tdma_steps(uint32_t* t, int k) {
    const tetra_lmac::Tdma r = handover::tdma_steps(tetra_lmac::Tdma{ t[0], t[1], t[2] }, k);
    t[0] = r.tn; t[1] = r.fn; t[2] = r.mn;
}

// The tail part of channel c's restart over the tables of restart_lanes.hpp's tail_view.  src < 0: a plain reset; else c is planted from
// src's anchor -- a donor (accept_pending = 0, elapsed = 0), or c itself after a gap of `elapsed` bits (accept_pending = 1).
void handover_emul_restart(State* states, uint8_t* carry, tetra_lmac::TrackState* cell, uint32_t* link, int link_words, int32_t* miss, Assist* assist, int c,
                           int src, int accept_pending, uint32_t elapsed, int window, int max_slots) {
    restart_emul::restart_channel(restart_emul::tail_view(states, carry, cell, link, link_words, miss, assist), c, src, accept_pending, elapsed, window, max_slots);
}

// The identity the single restart rests on, over every bits_in_buf 0 .. max_bits x window 0 .. max_window x the listed max_slots: a LOCKED
// channel with the cell cell10 (its bit buffer left out: nothing here reads it) restarted by two routes, as an heir of itself taken as a
// donor, and as its own heir after a gap of 0 bits.  Returns the number of cases in which State, Assist or cell differ between the two
// (first3: the first such case); *planted counts the cases in which both read ASSIST with the status PENDING.
long long handover_emul_own_donor_vs_resume(const uint32_t* cell10, int max_bits, int max_window, const int32_t* max_slots, int n_max_slots,
                                            long long* planted, int32_t* first3) {
    long long differing = 0;
    *planted = 0;
    for (int b = 0; b <= max_bits; ++b)
        for (int w = 0; w <= max_window; ++w)
            for (int k = 0; k < n_max_slots; ++k) {
                State st[2];
                Assist as[2];
                tetra_lmac::TrackState cell[2];
                int32_t miss[2] = { 3, 3 };
                for (int r = 0; r < 2; ++r) {
                    const uint32_t words[4] = { (uint32_t)kLocked, (uint32_t)b, 51000u, 51000u + (uint32_t)kTs };
                    std::memcpy(&st[r], words, sizeof words);
                    std::memset(&as[r], 0, sizeof as[r]);
                    std::memcpy(&cell[r], cell10, sizeof cell[r]);
                    restart_emul::restart_channel(restart_emul::tail_view(&st[r], nullptr, &cell[r], nullptr, 0, &miss[r], &as[r]), 0, 0, r, 0u, w, max_slots[k]);
                }
                if (st[0].state == (uint32_t)kAssist && as[0].status == kHoPending && st[1].state == (uint32_t)kAssist && as[1].status == kHoPending) ++*planted;
                if (std::memcmp(&st[0], &st[1], sizeof st[0]) || std::memcmp(&as[0], &as[1], sizeof as[0]) || std::memcmp(&cell[0], &cell[1], sizeof cell[0])) {
                    if (!differing) { first3[0] = b; first3[1] = w; first3[2] = max_slots[k]; }
                    ++differing;
                }
            }
    return differing;
}

void handover_emul_apply(Assist* assist, tetra_lmac::TrackState* cell, int n_channels) {
    for (int c = n_channels - 1; c >= 0; --c) handover::apply_channel(handover::View{ nullptr, assist, cell }, c);
}

}  // extern "C"
