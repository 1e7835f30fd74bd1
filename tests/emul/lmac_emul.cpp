// Host build of the lower-MAC decoder's lane-level code (sdrpp-tetra-demodulator_amd/csrc/lmac_core.hpp), one 64-row workgroup
// at a time with plain arrays behind the accessors the kernels put on LDS.  Every decoding entry is a loop over workgroups and lanes
// that picks one of lmac_core.hpp's block front ends -- the ones the kernels call -- and runs lmac_lane_io.hpp's lane epilogue behind
// it; k_lmac_decode's cooperative stage is lmac_lane_io.hpp's stage_workgroup.  Test infrastructure: lets the CPU suite check the exact
// kernel source, compositions included, against the reference-built primitives (oracle/_ref) without a GPU.
#define TETRA_HOST_EMUL 1
#include "lmac_lane_io.hpp"

using namespace lane_emul;

// k_lmac_decode, a 64-row workgroup at a time.  route: 0 = like the kernel (a workgroup whose rows are all plain bits, 8-byte aligned
// and at most 512 bytes apart takes the packed route, any other the byte route), 1 = byte route always (tetra_lmac_debug_force_byte_route).
// fast_rows: the rows of the workgroups that took the packed route.
extern "C" int lmac_emul_decode_route(int type345, int type2, int type1, int a, const uint8_t* type5, int n_blocks, int in_stride,
                                      const uint32_t* scramb_init, uint8_t* out, int out_stride, int32_t* crc_ok, int route, int32_t* fast_rows) {
    if (type345 > kMaxType345 || type2 > kMaxType2 || (type345 & 7) || (type2 & 15) || (in_stride & 3)) return -1;
    (void)type1;                  // n2 = type1 + 16 + 4 for every coded kind: the traceback derives the CRC span from n2
    const uint32_t* seq_tab = route == 0 ? seq_table() : nullptr;
    int fast = 0;
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        const uint8_t* rows = type5 + (size_t)blk0 * in_stride;
        uint32_t xb[kLanes][kSeqWords];
        OutW outw;
        const bool packed = stage_workgroup(seq_tab, type345, type5, rows, rows_here, in_stride, xb);
        if (packed) fast += rows_here;
        const BlockKind kind{ kLayoutNone, type345 };
        for (int lane = 0; lane < rows_here; ++lane) {
            const uint32_t code = scramb_init[blk0 + lane];
            uint32_t cls[kClsWords + 1];
            auto ld = [&](int w) { return cls[w]; };
            auto st = [&](int w, uint32_t word) { cls[w] = word; };
            auto no_count = [](bool) { return 0u; };
            if (packed) {
                descramble_words(type345, code, xb[lane], seq_rows(seq_tab), st);
                finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<true>(type345, type2, a, ld, io); }, no_count, NoRescue(), &crc_ok[blk0 + lane], nullptr, nullptr);
            } else {
                byte_row_block(&kind, code, row_words(rows + (size_t)lane * in_stride), st);
                finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<false>(type345, type2, a, ld, io); }, no_count, NoRescue(), &crc_ok[blk0 + lane], nullptr, nullptr);
            }
        }
        write_rows(outw, rows_here, type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    if (fast_rows) *fast_rows = fast;
    return 0;
}

// the front end alone: the packed words (xb [n_blocks][kSeqWords]) of every row of the workgroups that take the packed route, took[blk] =
// whether row blk's workgroup did
extern "C" void lmac_emul_stage(int type345, const uint8_t* type5, int n_blocks, int in_stride, uint32_t* xb_out, int32_t* took) {
    for (int blk0 = 0; blk0 < n_blocks; blk0 += kLanes) {
        const int rows_here = n_blocks - blk0 < kLanes ? n_blocks - blk0 : kLanes;
        uint32_t xb[kLanes][kSeqWords] = {};
        const bool packed = stage_workgroup(seq_table(), type345, type5, type5 + (size_t)blk0 * in_stride, rows_here, in_stride, xb);
        for (int lane = 0; lane < rows_here; ++lane) {
            took[blk0 + lane] = packed;
            std::memcpy(xb_out + (size_t)(blk0 + lane) * kSeqWords, xb[lane], sizeof(xb[lane]));
        }
    }
}
// lane_sequence alone: the words it hands out for a block of type345 bits under `code` (words [kSeqWords]); returns the mask of the
// words it handed out
extern "C" uint32_t lmac_emul_sequence(int type345, uint32_t code, uint32_t* words) {
    uint32_t mask = 0;
    lane_sequence(type345, code, seq_rows(seq_table()), [&](int w, uint32_t word) { words[w] = word; mask |= 1u << w; });
    return mask;
}
// unit_row (the multiply-shift row index of the front end and the write-back) for i = 0 .. n - 1
extern "C" void lmac_emul_unit_row(int units, int n, int32_t* out) {
    const uint32_t inv = unit_inverse(units);
    for (int i = 0; i < n; ++i) out[i] = unit_row(i, inv);
}
// blk_param(type) as type345, type2, type1, a, crc
extern "C" int lmac_emul_blk_param(int type, int32_t* out) {
    if (type < 0 || type > 5) return -1;
    const BlkParam& p = blk_param(type);
    const int32_t v[5] = { p.type345, p.type2, p.type1, p.a, p.crc };
    std::memcpy(out, v, sizeof(v));
    return 0;
}

// tetra_lmac_decode_frames_device, one job: the lane code of k_lmac_frames for every listed frame, a 64-row workgroup at a time.
// frames [n_frames][16] packed, frame_scramb per frame slot (NULL: SCRAMB_INIT).  out rows: type2 bits (BBK: 30 bits + 2 zero bytes).
extern "C" int lmac_emul_decode_frames(int tpsap, int blk_num, const uint32_t* frames, const int32_t* frame_type, const int32_t* row_frame,
                                       int n_rows, const uint32_t* frame_scramb, uint8_t* out, int out_stride, int32_t* crc_ok) {
    const int layout = tpsap < 0 || tpsap > 5 ? kLayoutNone : layout_for(tpsap, blk_num, false);
    if (layout == kLayoutNone) return -1;
    const BlkParam& p = blk_param(tpsap);
    const BlockKind kind{ layout, p.type345 };
    const uint32_t* seq_tab = seq_table();
    for (int blk0 = 0; blk0 < n_rows; blk0 += kLanes) {
        const int rows_here = n_rows - blk0 < kLanes ? n_rows - blk0 : kLanes;
        OutW outw;
        for (int lane = 0; lane < rows_here; ++lane) {
            const int blk = blk0 + lane;
            const FrameRef fr = frame_of(tpsap, row_frame, blk, frame_scramb);
            uint32_t fw[kFrameWords];
            load_frame(frame_rows(frames, fr.f), fw);
            if (layout == kLayoutBbk) {
                uint32_t seq = 0;
                lane_sequence(30, fr.code, seq_rows(seq_tab), [&](int w, uint32_t word) { seq = w == 0 ? word : seq; });
                const uint32_t y = (bbk_bits(fw, frame_type[fr.f]) ^ seq) & 0xfffffffcu;
                for (int k = 0; k < 8; ++k) { const uint32_t v = bbk_bytes(y, k); std::memcpy(out + (size_t)blk * out_stride + 4 * k, &v, 4); }
                crc_ok[blk] = 1;
                continue;
            }
            uint32_t cls[kSeqWords];
            frame_hard_block(&kind, fr.code, fw, [&] { return frame_type[fr.f]; }, seq_rows(seq_tab), [&](int w, uint32_t word) { cls[w] = word; });
            finish_lane(outw, lane, [&](LaneIo& io) { return decode_hard<true>(p.type345, p.type2, p.a, [&](int w) { return cls[w]; }, io); },
                        [](bool) { return 0u; }, NoRescue(), &crc_ok[blk], nullptr, nullptr);
        }
        if (layout != kLayoutBbk) write_rows(outw, rows_here, p.type2, out + (size_t)blk0 * out_stride, out_stride);
    }
    return 0;
}

// tdma_advance (the SB1 tracker's closed-form TDMA clock, lmac_core.hpp) for n start states (tn, fn, mn) and every k = 1..kmax:
// out[i][k - 1] = tdma_pack(tdma_advance(start i, k))
extern "C" void lmac_emul_tdma_advance(const uint32_t* start, int n, int kmax, uint32_t* out) {
    for (int i = 0; i < n; ++i)
        for (int k = 1; k <= kmax; ++k)
            out[(size_t)i * kmax + k - 1] = tdma_pack(tdma_advance(Tdma{ start[3 * i], start[3 * i + 1], start[3 * i + 2] }, (uint32_t)k));
}

// k_track's loop on the host, slot layout (tetra_lmac_track_sync_device): the SAME track_slot / track_carry / sync_pdu_words the kernel
// calls, with arrays where the kernel has ballots and lane shuffles.  cell [n_channels][10] = tetra_lmac_cell_state_t, in / out.
// stale_tcd_on_bad_crc != 0 plants the rule the tracker had before it was pinned to the reference (lmac_core.hpp: kStaleTcdOnBadCrc).
extern "C" void lmac_emul_track(const uint8_t* sb1, int stride, const int32_t* crc_ok, const int32_t* valid_in, const int32_t* n_frames, int n_channels,
                                int frames, uint32_t* cell, uint32_t* row_scramb, uint32_t* row_time_rx, uint32_t* row_time, int stale_tcd_on_bad_crc) {
    for (int c = 0; c < n_channels; ++c) {
        const int nf = n_frames ? (n_frames[c] < frames ? n_frames[c] : frames) : frames;
        uint32_t* cs = cell + (size_t)c * 10;
        TrackState st = { cs[0], cs[1], cs[2], cs[3], Tdma{ cs[4], cs[5], cs[6] }, Tdma{ cs[7], cs[8], cs[9] } };
        for (int f0 = 0; f0 < frames; f0 += kLanes) {
            uint32_t a[kLanes] = {}, b[kLanes] = {};
            unsigned long long mv = 0, mg = 0;
            for (int lane = 0; lane < kLanes; ++lane) {
                const int f = f0 + lane;
                const size_t r = (size_t)c * frames + f;
                const bool valid = f < frames && valid_in[r] != 0 && f < nf;
                if (valid) mv |= 1ull << lane;
                if (valid && crc_ok[r]) {
                    mg |= 1ull << lane;
                    const uint8_t* t2 = sb1 + r * stride;
                    sync_pdu_words([&](int k) -> uint32_t { return t2[4 * k] | (t2[4 * k + 1] << 8) | (t2[4 * k + 2] << 16) | ((uint32_t)t2[4 * k + 3] << 24); },
                                   a[lane], b[lane]);
                }
            }
            auto words = [&](int h, uint32_t& ah, uint32_t& bh) { ah = a[h]; bh = b[h]; };
            TrackSlot slot[kLanes];
            for (int lane = 0; lane < kLanes; ++lane)
                slot[lane] = stale_tcd_on_bad_crc ? track_slot<true>(st, mv, mg, lane, words) : track_slot<false>(st, mv, mg, lane, words);
            const int last_live = (nf - f0 < kLanes ? nf - f0 : kLanes) - 1;
            const uint32_t code_end = last_live < 0 ? st.scramb_init : slot[last_live].scramb;
            for (int lane = 0; lane < kLanes && f0 + lane < frames; ++lane) {
                const size_t r = (size_t)c * frames + f0 + lane;
                const bool live = f0 + lane < nf;
                row_scramb[r] = live ? slot[lane].scramb : code_end;
                row_time_rx[r] = live ? tdma_pack(slot[lane].t_rx) : 0u;
                row_time[r] = live ? tdma_pack(slot[lane].t_after) : 0u;
            }
            if (last_live >= 0) track_carry(st, slot[last_live]);
        }
        const uint32_t out[10] = { st.scramb_init, st.colour, st.mcc, st.mnc, st.tcd.tn, st.tcd.fn, st.tcd.mn, st.phy.tn, st.phy.fn, st.phy.mn };
        std::memcpy(cs, out, sizeof(out));
    }
}
