// What the host emulations of the burst synchroniser (bsync_emul.cpp, bsync_tol_emul.cpp) put around the lane code of
// sdrpp-tetra-demodulator_amd/csrc/bsync_core.hpp where k_burst_sync has LDS and barriers: one channel's call is one workgroup, its
// LDS plain arrays, its 256 threads a loop in descending order (no thread may depend on another's writes inside a step).
#pragma once
#include <cstdint>
#include <vector>

#include "../../sdrpp-tetra-demodulator_amd/csrc/bsync_core.hpp"

namespace bsync_emul {

using namespace bsync_core;

template <class F> void for_threads(F f) {
    for (int t = kThreads - 1; t >= 0; --t) f(t);
}

struct Call {
    int n_new, max_frames;
    std::vector<uint32_t> s;            // the packed stream; starts out as all ones: the kernel's LDS is not cleared
    std::vector<FrameRec> rec;

    // step 1: the carried buffer and the new bits, every word by stage_thread
    Call(const State& st, const uint8_t* carry, const uint8_t* bits, int n_new_, int max_bits, int max_frames_)
        : n_new(n_new_), max_frames(max_frames_), s(stream_words(max_bits), 0xffffffffu), rec(max_frames_ > 0 ? max_frames_ : 0) {
        for_threads([&](int t) { stage_thread(t, s.data(), (int)s.size(), kOff - (int)st.bits_in_buf, n_new, carry, bits); });
    }
    // walk()'s emit, as the kernel lists a frame
    void emit(int f, int bx, int type, uint32_t bitnum) {
        if (f < max_frames) rec[f] = FrameRec{ bx, type, bitnum };
    }
    // step 4 for every thread: nf listed frames ([max_frames][16] words if packed, else [max_frames][512] bytes), the types and bit
    // numbers of all max_frames slots, the carried buffer from carry_x on
    void write(int nf, int carry_x, int packed, uint8_t* carry, void* frames, int32_t* types, uint32_t* bitnums, int none_type) const {
        for_threads([&](int t) {
            if (packed) write_thread<true>(t, s.data(), rec.data(), nf, max_frames, none_type, carry_x, kOff + n_new, static_cast<uint8_t*>(frames), types, bitnums, carry);
            else write_thread<false>(t, s.data(), rec.data(), nf, max_frames, none_type, carry_x, kOff + n_new, static_cast<uint8_t*>(frames), types, bitnums, carry);
        });
    }
    // steps 3 and 4: walk_rule(carry_x, first, emit) is run() or run_tolerant() on this call's stream with the emulation's bitmaps and
    // its form of the LOCKED batch; it gets the host's first_set and emit.  Returns the frame count, or -1 if more frames were consumed
    // than max_frames (the first max_frames are written).
    template <class WalkRule>
    int finish(WalkRule walk_rule, int packed, uint8_t* carry, void* frames, int32_t* types, uint32_t* bitnums) {
        int carry_x = 0;
        const int n = walk_rule(carry_x, [](const uint32_t* m, int a, int b) { return first_set(m, a, b); },
                                [&](int f, int bx, int type, uint32_t bitnum) { emit(f, bx, type, bitnum); });
        write(n < max_frames ? n : max_frames, carry_x, packed, carry, frames, types, bitnums, -2 /* TETRA_FRAME_NONE */);
        return n > max_frames ? -1 : n;
    }
};

}  // namespace bsync_emul
