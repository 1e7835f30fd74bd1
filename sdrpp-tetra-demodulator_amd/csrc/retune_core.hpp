// retune_core.hpp -- lane code of the per-channel resets behind include/tetra_retune.h: what tetra_rx_reset leaves in EVERY channel,
// written into the channels of a list.  Host- and device-callable (tests/emul/retune_emul.cpp runs it on the host); plain stores only.
//
// The views name the stages' per-channel state where the stages keep it (tetra_demod.hip: struct tetra_demod, tetra_burst_sync.hip:
// struct tetra_bsync, rx_handle.hpp: cell).  Complex arrays are addressed as floats, two per sample.  One channel is reset by
// `lanes` lanes together: lane 0 writes the scalars, all lanes stride over the arrays.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace retune {

struct DemodView {
    float *agc_g, *fll_ph, *fll_fr, *mu, *omega, *cph, *cfr, *ph2;
    int32_t *offset, *prev, *rrc_valid;
    float *hist, *hist_far, *ybuf;            // [C][2 n_hist], [C][2 n_hist_far], [C][2 n_ybuf]
    float* q_ring;                            // TETRA_FLAG_QUALITY: [C][n_q_ring] (null without the flag, with the four below)
    int32_t *q_ptr, *q_disp, *q_sync;
    float* q_err;
    float* cd_blk;                            // TETRA_FLAG_CONSTELLATION: [C][2 n_cd] (null without the flag, with the two below)
    int32_t *cd_fill, *cd_blocks;
    int32_t n_hist, n_hist_far, n_ybuf, n_q_ring, n_cd;
    int32_t rrc_all;                          // rrc_valid of a fresh channel: the longest delay line any kernel keeps
    float tr_omega;                           // the timing loop's nominal samples per symbol (the design's)
    int32_t fresh;                            // 0 under TETRA_FLAG_REFERENCE_QUIRKS: PI4DQPSK::reset to the letter (see reset_range)
};

struct BsyncView {
    uint32_t* state;                          // [C][state_words]: the synchroniser's State
    uint32_t* carry;                          // [C][carry_words]: its bit buffer, one byte per bit
    int32_t state_words, carry_words;
};

struct CellView {
    uint32_t* cell;                           // [C][cell_words]: tetra_lmac_cell_state_t
    int32_t cell_words;
};

struct SoftView {                             // TETRA_RX_FLAG_SOFT (rx_handle.hpp; all null without the flag)
    float* prev;                              // [2][C][2]: a channel's previous symbol, both parities
    uint32_t* bits;                           // [2][C]: its absolute bit count
    int32_t n_channels;
    float fresh_prev;                         // both components of a fresh channel's previous symbol
};

RT_HD void zero_f32(float* p, long long n, int lane, int lanes) {
    for (long long i = lane; i < n; i += lanes) p[i] = 0.0f;
}
RT_HD void zero_u32(uint32_t* p, long long n, int lane, int lanes) {
    for (long long i = lane; i < n; i += lanes) p[i] = 0u;
}

// tetra_demod.hip's reset_range for channel c: PI4DQPSK::reset (pi4dqpsk.cpp:120-130), and with `fresh` everything that reset leaves
// alone too (delay lines, ph2, the slicer's previous symbol, COMPLEX_FD's buffer, the quality and constellation taps).
RT_HD void reset_demod_channel(const DemodView& v, int c, int lane, int lanes) {
    if (lane == 0) {
        v.agc_g[c] = 1.0f;
        v.fll_ph[c] = 0.0f;
        v.fll_fr[c] = 0.0f;
        v.rrc_valid[c] = v.fresh ? v.rrc_all : 0;
        v.mu[c] = 0.0f;
        v.omega[c] = v.tr_omega;
        v.offset[c] = 0;
        v.cph[c] = 0.0f;
        v.cfr[c] = 0.0f;
    }
    if (!v.fresh) return;
    if (lane == 0) {
        v.ph2[c] = 0.0f;
        v.prev[c] = 0;
        if (v.q_ring) {
            v.q_ptr[c] = 0;
            v.q_disp[c] = 0;
            v.q_sync[c] = 0;
            v.q_err[c] = 0.0f;
        }
        if (v.cd_blk) {
            v.cd_fill[c] = 0;
            v.cd_blocks[c] = 0;
        }
    }
    zero_f32(v.hist + (long long)c * 2 * v.n_hist, 2LL * v.n_hist, lane, lanes);
    zero_f32(v.hist_far + (long long)c * 2 * v.n_hist_far, 2LL * v.n_hist_far, lane, lanes);
    zero_f32(v.ybuf + (long long)c * 2 * v.n_ybuf, 2LL * v.n_ybuf, lane, lanes);
    if (v.q_ring) zero_f32(v.q_ring + (long long)c * v.n_q_ring, v.n_q_ring, lane, lanes);
    if (v.cd_blk) zero_f32(v.cd_blk + (long long)c * 2 * v.n_cd, 2LL * v.n_cd, lane, lanes);
}

// the soft-decision quantiser's carried state of channel c: bit numbering from 0 like the synchroniser's, no previous symbol
RT_HD void reset_soft_channel(const SoftView& v, int c, int lane, int lanes) {
    (void)lanes;
    if (!v.prev || lane >= 2) return;
    const long long at = (long long)lane * v.n_channels + c;      // lane = parity
    v.prev[2 * at] = v.fresh_prev;
    v.prev[2 * at + 1] = v.fresh_prev;
    v.bits[at] = 0u;
}

// tetra_bsync_reset for channel c: UNLOCKED, no bits, bit numbering from 0
RT_HD void reset_bsync_channel(const BsyncView& v, int c, int lane, int lanes) {
    zero_u32(v.state + (long long)c * v.state_words, v.state_words, lane, lanes);
    zero_u32(v.carry + (long long)c * v.carry_words, v.carry_words, lane, lanes);
}

// the chain's cell state and TDMA clock of channel c: the reference's zero-initialised tcd / t_phy_state
RT_HD void reset_cell_channel(const CellView& v, int c, int lane, int lanes) {
    zero_u32(v.cell + (long long)c * v.cell_words, v.cell_words, lane, lanes);
}

// The tail's per-channel tables, all of them: what a restart of a channel clears behind the demodulator.  A table the handle does not
// keep, or miss counters that the rule in force does not count, has zero words and is skipped.
struct TailView {
    BsyncView sync;                           // the synchroniser's State and bit buffer
    CellView cell;                            // tetra_lmac_cell_state_t
    CellView link;                            // tetra_rx_link_t (TETRA_RX_FLAG_BITERR)
    CellView miss;                            // the tolerant lock's miss counter (tetra_sync_tol.h)
    CellView assist;                          // the hand-over fields (bsync_core.hpp: Assist), from a handle's first hand-over or gap on
};

// Every table of TailView for channel c.  The list of tables exists here and nowhere else: the kernel and the host emulations call this.
RT_HD void reset_tail_channel(const TailView& v, int c, int lane, int lanes) {
    reset_bsync_channel(v.sync, c, lane, lanes);
    reset_cell_channel(v.cell, c, lane, lanes);
    reset_cell_channel(v.link, c, lane, lanes);
    reset_cell_channel(v.miss, c, lane, lanes);
    reset_cell_channel(v.assist, c, lane, lanes);
}

// The wideband receiver's history ring: the channeliser's newest `hist` frames of all M bins, frame a (counted from the stream's
// start) in row a mod hist.  keep_row: element i of the `rows` newest frames of a call that brought n_in frames after n0 earlier ones.
RT_HD void keep_element(const float* x, int M, long long n0, int n_in, int rows, int hist, long long i, float* ring) {
    const long long r = i / M;
    const int k = (int)(i - r * M);
    const long long f = (long long)n_in - rows + r;             // the frame's row in x
    const long long at = ((n0 + f) % hist) * M + k;
    ring[2 * at] = x[2 * (f * M + k)];
    ring[2 * at + 1] = x[2 * (f * M + k) + 1];
}

// Delay-line row r (0 = oldest of the hist frames before frame n_total) of slot `slot` from the ring's column `bin`; frames before
// the stream's start are zeros, as in a resampler that has just been created.
RT_HD void rebuild_element(const float* ring, int M, int hist, long long n_total, int r, int bin, int slot, int C, float* line) {
    const long long a = n_total - hist + r;
    float re = 0.0f, im = 0.0f;
    if (a >= 0) {
        const long long at = (a % hist) * M + bin;
        re = ring[2 * at];
        im = ring[2 * at + 1];
    }
    line[2 * ((long long)r * C + slot)] = re;
    line[2 * ((long long)r * C + slot) + 1] = im;
}

}  // namespace retune
