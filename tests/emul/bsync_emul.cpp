// Host build of the burst synchroniser's logic (sdrpp-tetra-demodulator_amd/csrc/bsync_core.hpp): same event-driven
// state machine, bitmaps and literal fallback as the kernel, with the kernel's parallel phases done sequentially.
// Test infrastructure: checked against the literal restatement fed one bit per call (oracle/burst_sync_oracle.c).
#define TETRA_HOST_EMUL 1
#include <cstdint>
#include <cstring>
#include <vector>

#include "bsync_lane_io.hpp"

using namespace bsync_core;

namespace {
int process(State* st, uint8_t* carry, const uint8_t* bits, int n_new, void* frames, int packed, int32_t* types, uint32_t* bitnums, int max_frames,
            int use_batch) {
    bsync_emul::Call call(*st, carry, bits, n_new, n_new, max_frames);
    const int words = (int)call.s.size(), x0 = kOff - (int)st->bits_in_buf, xe = kOff + n_new;
    const uint32_t* s = call.s.data();
    std::vector<uint32_t> ms(words, 0), m1(words, 0), m2(words, 0), ma(words, 0);
    for (int w = x0 >> 5; w <= (xe - 1) >> 5 && w + 2 < words; ++w) { match_word(s, w, x0, xe, ms[w], m1[w], m2[w]); ma[w] = ms[w] | m1[w] | m2[w]; }
    // the kernel's batch of LOCKED frames (one per lane, 64 per round, stopping behind the first frame that unlocks), frame by frame
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
    return call.finish([&](int& carry_x, auto first, auto emit) {
        return run(*st, s, ms.data(), m1.data(), m2.data(), ma.data(), n_new, carry_x, first, emit, batch);
    }, packed, carry, frames, types, bitnums);
}
}  // namespace

// frames [max_frames][512] bytes
extern "C" int bsync_emul_process(State* st, uint8_t* carry, const uint8_t* bits, int n_new, uint8_t* frames, int32_t* types,
                                  uint32_t* bitnums, int max_frames, int use_batch) {
    return process(st, carry, bits, n_new, frames, 0, types, bitnums, max_frames, use_batch);
}
// frames [max_frames][16] words
extern "C" int bsync_emul_process_packed(State* st, uint8_t* carry, const uint8_t* bits, int n_new, uint32_t* frames, int32_t* types,
                                         uint32_t* bitnums, int max_frames, int use_batch) {
    return process(st, carry, bits, n_new, frames, 1, types, bitnums, max_frames, use_batch);
}

// steps 1 and 4 on their own (tests/test_burst_sync.py holds them against their definitions).
// the packed stream of a call: stream_words(max_bits) words
extern "C" int bsync_emul_stage(int bits_in_buf, const uint8_t* carry, const uint8_t* bits, int n_new, int max_bits, uint32_t* s_out) {
    const State st = { 0, (uint32_t)bits_in_buf, 0, 0 };
    const bsync_emul::Call call(st, carry, bits, n_new, max_bits, 0);
    std::memcpy(s_out, call.s.data(), call.s.size() * sizeof(uint32_t));
    return (int)call.s.size();
}
// the frames that start at bx[0 .. nf) of that stream, and the carried buffer from carry_x on
extern "C" void bsync_emul_expand(int bits_in_buf, const uint8_t* carry_in, const uint8_t* bits, int n_new, int max_bits, const int32_t* bx, int nf,
                                  int carry_x, int packed, void* frames, int32_t* types, uint32_t* bitnums, uint8_t* carry_out) {
    const State st = { 0, (uint32_t)bits_in_buf, 0, 0 };
    bsync_emul::Call call(st, carry_in, bits, n_new, max_bits, nf);
    for (int f = 0; f < nf; ++f) call.emit(f, bx[f], f & 3, (uint32_t)bx[f]);
    call.write(nf, carry_x, packed, carry_out, frames, types, bitnums, -2);
}

// ---- the demultiplexer kernels (csrc/demux_core.hpp): every (workgroup, thread) of the launch tetra_burst_sync.hip's launchers would
// make, in turn (threads descending inside a workgroup, workgroups ascending: no thread may depend on another's writes) -------------
#include "../../sdrpp-tetra-demodulator_amd/csrc/demux_core.hpp"

namespace {
template <class F> void for_grid(long long blocks, F f) {
    for (long long b = 0; b < blocks; ++b)
        for (int t = demux_core::kThreads - 1; t >= 0; --t) f((uint32_t)b, (uint32_t)t);
}
}  // namespace

// frames: [n][512] bytes or, packed != 0, [n][16] words.  Returns 0, or -1 for arguments the launchers refuse.
extern "C" int bsync_emul_demux(const uint8_t* frames, int packed, const int32_t* frame_type, int n, int tpsap, int blk_num, uint8_t* rows,
                                int row_stride, int32_t* valid) {
    using namespace demux_core;
    const PiecesLut lut = lut_for(tpsap, blk_num);
    int longest = 0;
    for (const Pieces* p : { &lut.sync, &lut.norm1, &lut.norm2 }) longest = p->len0 + p->len1 > longest ? p->len0 + p->len1 : longest;
    if (longest == 0 || row_stride < longest || (row_stride & 3)) return -1;
    const bool wide = !(row_stride & 7) && !((uintptr_t)rows & 7);
    if (use_rows_kernel(packed != 0, wide, row_stride)) {
        const int row_u = row_stride >> 3, rpw = 64 / row_u;
        for_grid(rows_grid(n, row_stride), [&](uint32_t b, uint32_t t) {
            rows_thread<false>(b, t, frames, frame_type, nullptr, n, lut, row_u, rpw, (uint32_t)((65536 + row_u - 1) / row_u), rows, valid);
        });
        return 0;
    }
    for_grid(units_grid(n, row_stride, wide), [&](uint32_t b, uint32_t t) {
        if (packed && wide) demux_thread<true, true>(b, t, frames, frame_type, n, tpsap, blk_num, rows, row_stride, valid);
        else if (packed) demux_thread<true, false>(b, t, frames, frame_type, n, tpsap, blk_num, rows, row_stride, valid);
        else if (wide) demux_thread<false, true>(b, t, frames, frame_type, n, tpsap, blk_num, rows, row_stride, valid);
        else demux_thread<false, false>(b, t, frames, frame_type, n, tpsap, blk_num, rows, row_stride, valid);
    });
    return 0;
}

// the compacting form: row_frame / n_rows as the list passes (k_list_count / _scan / _write with CarriesKind) leave them (frame order), then the gather
extern "C" int bsync_emul_demux_compact(const uint8_t* frames, int packed, const int32_t* frame_type, int n, int tpsap, int blk_num,
                                        uint8_t* rows, int row_stride, int32_t* row_frame, int32_t* n_rows) {
    using namespace demux_core;
    const PiecesLut lut = lut_for(tpsap, blk_num);
    int longest = 0;
    for (const Pieces* p : { &lut.sync, &lut.norm1, &lut.norm2 }) longest = p->len0 + p->len1 > longest ? p->len0 + p->len1 : longest;
    if (longest == 0 || row_stride < longest || (row_stride & 3)) return -1;
    int cnt = 0;
    for (int r = 0; r < n; ++r)
        if (pieces_for(frame_type[r], tpsap, blk_num).len0 > 0) row_frame[cnt++] = r;
    *n_rows = cnt;
    const bool wide = !(row_stride & 7) && !((uintptr_t)rows & 7);
    if (use_rows_kernel(packed != 0, wide, row_stride)) {
        const int row_u = row_stride >> 3, rpw = 64 / row_u;
        for_grid(rows_grid(n, row_stride), [&](uint32_t b, uint32_t t) {
            rows_thread<true>(b, t, frames, frame_type, row_frame, cnt, lut, row_u, rpw, (uint32_t)((65536 + row_u - 1) / row_u), rows, nullptr);
        });
        return 0;
    }
    for_grid(units_grid(n, row_stride, wide), [&](uint32_t b, uint32_t t) {
        if (packed && wide) gather_thread<true, true>(b, t, frames, frame_type, row_frame, cnt, n, tpsap, blk_num, rows, row_stride);
        else if (packed) gather_thread<true, false>(b, t, frames, frame_type, row_frame, cnt, n, tpsap, blk_num, rows, row_stride);
        else if (wide) gather_thread<false, true>(b, t, frames, frame_type, row_frame, cnt, n, tpsap, blk_num, rows, row_stride);
        else gather_thread<false, false>(b, t, frames, frame_type, row_frame, cnt, n, tpsap, blk_num, rows, row_stride);
    });
    return 0;
}
