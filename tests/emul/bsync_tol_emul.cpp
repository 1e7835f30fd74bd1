// Host build of the burst synchroniser's tolerant lock (sdrpp-tetra-demodulator_amd/csrc/bsync_core.hpp: run_tolerant, tolerant_frame_eval,
// first_unlock / first_unlock_bits; include/ext/tetra_sync_tol.h), with the kernel's parallel phases done sequentially: the sync bitmap
// word by word, the LOCKED batch in rounds of 64 frames whose reported bits form the mask the kernel gets from its ballot.
// Test infrastructure: checked against the restatement in tests/test_sync_tol.py, fed one bit per call.
#define TETRA_HOST_EMUL 1
#include <cstdint>
#include <cstring>
#include <vector>

#include "bsync_lane_io.hpp"

using namespace bsync_core;

// mode 0: no batch (every LOCKED call through the event path); 1: batch, consecutive-miss rule by first_unlock (the loop);
// 2: batch, first_unlock_bits (the kernel's).  tol3 = {tol_norm, tol_sync, max_miss}.  Returns the frame count, -1 on overflow, -2 for
// a tolerance out of range.
namespace {
int process(State* st, int32_t* misses, uint8_t* carry, const uint8_t* bits, int n_new, const int32_t* tol3, void* frames, int packed, int32_t* types,
            uint32_t* bitnums, int max_frames, int mode) {
    const Tolerance tol = { tol3[0], tol3[1], tol3[2] };
    if (!tolerance_valid(tol)) return -2;
    bsync_emul::Call call(*st, carry, bits, n_new, n_new, max_frames);
    const int words = (int)call.s.size(), x0 = kOff - (int)st->bits_in_buf, xe = kOff + n_new;
    const uint32_t* s = call.s.data();
    std::vector<uint32_t> ms(words, 0);
    for (int w = x0 >> 5; w <= (xe - 1) >> 5 && w + 2 < words; ++w) ms[w] = match_word_sync(s, w, x0, xe);
    int m = *misses;
    auto batch = [&](int bx, int K, int f0, uint32_t abs_bx, bool& unlocked) {
        if (!mode) return 0;
        int done = 0;
        while (done < K) {
            const int here = K - done < 64 ? K - done : 64;
            int reported[64];
            uint64_t pass = 0;
            for (int lane = 0; lane < 64; ++lane) {              // (lanes past `here` report nothing, as in the kernel's ballot)
                reported[lane] = lane < here ? tolerant_frame_eval(s, bx + kTs * (done + lane), tol) : -1;
                if (reported[lane] >= 0) pass |= 1ull << lane;
            }
            const Unlock u = mode == 2 ? first_unlock_bits(pass, here, m, tol.max_miss) : first_unlock(pass, here, m, tol.max_miss);
            const int take = u.index >= 0 ? u.index + 1 : here;
            for (int lane = 0; lane < take; ++lane) call.emit(f0 + done + lane, bx + kTs * (done + lane), reported[lane], abs_bx + (uint32_t)(kTs * (done + lane)));
            m = u.misses;
            done += take;
            if (u.index >= 0) { unlocked = true; break; }
        }
        return done;
    };
    const int n = call.finish([&](int& carry_x, auto first, auto emit) { return run_tolerant(*st, s, ms.data(), n_new, carry_x, first, emit, batch, tol, m); },
                              packed, carry, frames, types, bitnums);
    *misses = m;
    return n;
}
}  // namespace

// frames [max_frames][512] bytes
extern "C" int bsync_tol_emul_process(State* st, int32_t* misses, uint8_t* carry, const uint8_t* bits, int n_new, const int32_t* tol3, uint8_t* frames,
                                      int32_t* types, uint32_t* bitnums, int max_frames, int mode) {
    return process(st, misses, carry, bits, n_new, tol3, frames, 0, types, bitnums, max_frames, mode);
}
// frames [max_frames][16] words
extern "C" int bsync_tol_emul_process_packed(State* st, int32_t* misses, uint8_t* carry, const uint8_t* bits, int n_new, const int32_t* tol3,
                                             uint32_t* frames, int32_t* types, uint32_t* bitnums, int max_frames, int mode) {
    return process(st, misses, carry, bits, n_new, tol3, frames, 1, types, bitnums, max_frames, mode);
}

// out = {index, misses}
extern "C" void bsync_tol_emul_first_unlock(uint64_t pass_mask, int n, int misses_in, int max_miss, int bits, int32_t* out) {
    const Unlock u = bits ? first_unlock_bits(pass_mask, n, misses_in, max_miss) : first_unlock(pass_mask, n, misses_in, max_miss);
    out[0] = u.index;
    out[1] = u.misses;
}

// many at once: masks [count], n / misses_in / max_miss [count] -> out [count][2]
extern "C" void bsync_tol_emul_first_unlock_many(const uint64_t* pass_mask, const int32_t* n, const int32_t* misses_in, const int32_t* max_miss, int count,
                                                 int bits, int32_t* out) {
    for (int i = 0; i < count; ++i) bsync_tol_emul_first_unlock(pass_mask[i], n[i], misses_in[i], max_miss[i], bits, out + 2 * i);
}

// tolerant_frame_eval on one frame of 510 bits (one byte per bit)
extern "C" int bsync_tol_emul_frame_eval(const uint8_t* frame, const int32_t* tol3) {
    uint32_t s[20] = {};
    for (int i = 0; i < kTs; ++i) s[i >> 5] |= (uint32_t)(frame[i] & 1u) << (31 - (i & 31));
    return tolerant_frame_eval(s, 0, Tolerance{ tol3[0], tol3[1], tol3[2] });
}
