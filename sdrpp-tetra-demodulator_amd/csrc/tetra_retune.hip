// tetra_retune.hip -- retuning while the stream runs (include/tetra_retune.h): the stream-ordered reset of listed channels of the
// receive chain, and the wideband receiver's retune of carrier slots on top of it.
//
// Nothing here waits on the host.  Two calls may be in flight (the demodulator of call k + 1 runs beside the tail of call k), so a
// reset between call k and call k + 1 is split by stream:
//
//   caller's stream  [wait: demodulator k]  (wideband: bin list, delay-line columns)  k_reset_demod           (event ev_reset)
//   tail stream      [behind tail k, wait ev_reset]  k_reset_tail: synchroniser state + bit buffer, cell state
//
// and call k + 1 is ordered behind both: its demodulator waits for ev_reset, its tail runs on the tail stream.  The events of call k
// (ev_demod, ev_tail, the wideband ev_done) are recorded again behind the reset, so whoever waits for that call -- tetra_rx_wait,
// the state readers, the call after next -- also waits for the reset.  Call k's results are not touched: they stay fetchable.
//
// The kernels are a launch of one 64-lane workgroup per listed channel (lane code: retune_core.hpp): not a hot path.
// A reset with donors (include/ext/tetra_handover.h) is the same reset with one more kernel behind k_reset_tail on the tail stream,
// k_handover_plant (lane code: handover_core.hpp), which reads the donors' state as the last tail left it.
// A stream gap (include/ext/tetra_gap.h) is the same reset with k_resume_tail in place of k_reset_tail: each listed channel reads its own
// state before it clears it and resumes as its own heir.  The wideband handle's gap puts the front end's restart in front, on the
// caller's stream: what tetra_wbrx_reset leaves, without its host synchronisation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/ext/tetra_gap.h"
#include "../../include/ext/tetra_handover.h"
#include "../../include/tetra_retune.h"
#include "handover_core.hpp"
#include "hip_host.hpp"
#include "resamp_handle.hpp"
#include "retune_core.hpp"
#include "retune_impl.hpp"
#include "rx_handle.hpp"
#include "soft_core.hpp"
#include "wbrx_handle.hpp"

namespace {

constexpr int kLanes = 64;

__global__ __launch_bounds__(kLanes) void k_reset_demod(retune::DemodView v, retune::SoftView soft, const int32_t* __restrict__ channels, int n_channels) {
    const int c = channels[blockIdx.x];
    if (c < 0 || c >= n_channels) return;          // (the host has checked the list)
    retune::reset_demod_channel(v, c, threadIdx.x, kLanes);
    retune::reset_soft_channel(soft, c, threadIdx.x, kLanes);
}

// link: the channels' link figures as words (tetra_rx_link_t, TETRA_RX_FLAG_BITERR; no words without the flag), zeroed like the cell state
__global__ __launch_bounds__(kLanes) void k_reset_tail(retune::BsyncView b, retune::CellView cell, retune::CellView link, const int32_t* __restrict__ channels,
                                                       int n_channels) {
    const int c = channels[blockIdx.x];
    if (c < 0 || c >= n_channels) return;
    retune::reset_bsync_channel(b, c, threadIdx.x, kLanes);
    retune::reset_cell_channel(cell, c, threadIdx.x, kLanes);
    retune::reset_cell_channel(link, c, threadIdx.x, kLanes);
}

// the synchroniser's miss counters under the tolerant lock (tetra_sync_tol.h), one word per channel: a launch of its own behind
// k_reset_tail, made only for a chain that runs that rule
__global__ __launch_bounds__(kLanes) void k_reset_miss(retune::CellView miss, const int32_t* __restrict__ channels, int n_channels) {
    const int c = channels[blockIdx.x];
    if (c < 0 || c >= n_channels) return;
    retune::reset_cell_channel(miss, c, threadIdx.x, kLanes);
}

// The hand-over's planting (include/ext/tetra_handover.h; lane code: handover_core.hpp), behind k_reset_tail and the reset of the listed
// channels' Assist: a thread per entry, heirs[i] from donors[i] (-1: a plain restart).  The host has checked that no donor is an heir.
__global__ __launch_bounds__(kLanes) void k_handover_plant(handover::View v, const int32_t* __restrict__ heirs, const int32_t* __restrict__ donors, int n,
                                                           int n_channels, int32_t window, int32_t max_slots) {
    const int i = (int)blockIdx.x * kLanes + (int)threadIdx.x;
    if (i >= n) return;
    const int c = heirs[i], d = donors[i];
    if (c < 0 || c >= n_channels || d < 0 || d >= n_channels) return;
    handover::plant_channel(v, c, d, window, max_slots);
}

// A stream gap (include/ext/tetra_gap.h; lane code: handover_core.hpp): the tail part of a listed channel's restart as its own heir, in
// one launch in place of k_reset_tail and the resets behind it.  Every lane reads the channel's anchor before any lane clears the
// channel; lane 0 plants behind the clearing.  miss: zero words where the rule in force counts none.
__global__ __launch_bounds__(kLanes) void k_resume_tail(retune::BsyncView b, retune::CellView cell, retune::CellView link, retune::CellView miss,
                                                        retune::CellView assist, const int32_t* __restrict__ channels, int n_channels, uint32_t elapsed,
                                                        int32_t window, int32_t max_slots) {
    const int c = channels[blockIdx.x];
    if (c < 0 || c >= n_channels) return;
    const handover::View v = { reinterpret_cast<bsync_core::State*>(b.state), reinterpret_cast<bsync_core::Assist*>(assist.cell),
                               reinterpret_cast<tetra_lmac::TrackState*>(cell.cell) };
    const handover::Anchor an = handover::gap_anchor(v, c);
    __syncthreads();
    retune::reset_bsync_channel(b, c, threadIdx.x, kLanes);
    retune::reset_cell_channel(cell, c, threadIdx.x, kLanes);
    retune::reset_cell_channel(link, c, threadIdx.x, kLanes);
    retune::reset_cell_channel(miss, c, threadIdx.x, kLanes);
    retune::reset_cell_channel(assist, c, threadIdx.x, kLanes);
    __syncthreads();
    if (threadIdx.x == 0) handover::resume_channel(v, c, an, elapsed, window, max_slots);
}

// list = [n slots | n bins]: bins[slot_i] = bin_i, and the slot's column of the resampler's delay line line [hist][C] from the
// history ring [hist][M] (a sibling of tetra_resamp.hip's k_pick_rows: same rows, one column each, out of the ring)
__global__ __launch_bounds__(256) void k_retune_columns(const float* __restrict__ ring, int M, int hist, long long n_total, const int32_t* __restrict__ list,
                                                        int n, int C, float* __restrict__ line, int32_t* __restrict__ bins) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hist * n) return;
    const int r = i / n, j = i - r * n;
    const int slot = list[j], bin = list[n + j];
    if (slot < 0 || slot >= C || bin < 0 || bin >= M) return;
    retune::rebuild_element(ring, M, hist, n_total, r, bin, slot, C, line);
    if (r == 0) bins[slot] = bin;
}

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

// false: an index outside [0, limit) or twice in the list
bool distinct_in_range(const int32_t* v, int n, int limit) {
    std::vector<char> seen((size_t)limit, 0);
    for (int i = 0; i < n; i++) {
        if (v[i] < 0 || v[i] >= limit || seen[(size_t)v[i]]) return false;
        seen[(size_t)v[i]] = 1;
    }
    return true;
}

// a hand-over's parameters, or the defaults; false: out of range
bool handover_params(const tetra_handover_params_t* p, tetra_handover_params_t* out) {
    *out = p ? *p : tetra_handover_params_t{ TETRA_HANDOVER_DEFAULT_WINDOW, TETRA_HANDOVER_DEFAULT_MAX_SLOTS };
    return out->window >= 0 && out->window <= bsync_core::kWindowMax && out->max_slots >= 1 && out->max_slots <= bsync_core::kAssistSlotsMax;
}

// a gap's parameters, or its header's defaults; false: out of range
bool gap_params(const tetra_handover_params_t* p, tetra_handover_params_t* out) {
    const tetra_handover_params_t def = { TETRA_GAP_DEFAULT_WINDOW, TETRA_GAP_DEFAULT_MAX_SLOTS };
    return handover_params(p ? p : &def, out);
}

// The chain's part, for n > 0 channels listed on the device at d_channels (uploaded on s).  The caller marks the list's readers:
// s, and *tail_reader (the tail stream when the chain has one of its own, else null).
// d_donors (may be null: a plain reset): per listed channel its donor or -1, planted behind the reset with the parameters *p.
// elapsed (may be null; never with donors): a stream gap of *elapsed bits -- every listed channel resumes as its own heir with *p.
int reset_enqueue(tetra_rx* h, const int32_t* d_channels, int n, hipStream_t s, hipStream_t* tail_reader, const int32_t* d_donors = nullptr,
                  const tetra_handover_params_t* p = nullptr, const uint32_t* elapsed = nullptr) {
    retune::DemodView dv;
    retune::BsyncView bv;
    TETRA_TRY(retune_impl::demod_view(h->dem, &dv));
    TETRA_TRY(retune_impl::bsync_view(h->bs, &bv));
    static_assert(sizeof(tetra_lmac_cell_state_t) % 4 == 0 && sizeof(tetra_rx_link_t) % 4 == 0, "reset in 32-bit words");
    // the chain's per-channel tables in 32-bit words per channel: no words where the handle has no such table, nor for miss counters
    // that the rule in force does not count
    retune::CellView tv[kChanTablesAll];
    for (int t = 0; t < kChanTablesAll; ++t) {
        void* at = nullptr;
        bool counting = true;
        TETRA_TRY(chan_tab::live(h, t, &at, &counting));
        tv[t] = { static_cast<uint32_t*>(at), at && counting ? (int32_t)(chan_tab::elem_bytes(t) / 4) : 0 };
    }
    const retune::CellView &cv = tv[TAB_CELL], &lv = tv[TAB_LINK], &mv = tv[TAB_SYNC_MISSES], &av = tv[TAB_HANDOVER];
    if (!h->ev_reset) HIP_TRY(h, hipEventCreateWithFlags(h->ev_reset.put(), hipEventDisableTiming));
    const int last = (int)((h->calls - 1) & 1);
    hipStream_t st = h->one_stream ? s : static_cast<hipStream_t>(h->tail);
    if (h->reset_pending) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_reset, 0));        // an earlier reset, possibly given another stream
    if (h->calls > 0) {
        HIP_TRY(h, hipStreamWaitEvent(s, h->ev_demod[last], 0));
        // (soft decisions: a reset channel's bit numbering restarts, so the next call's soft values land anywhere in its ring -- where the
        //  last call's tail may still be reading: the reset, and with it that call, waits for the tail)
        if (h->one_stream || h->soft) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_tail[last], 0));
    }
    const retune::SoftView sv = { h->soft_prev.get(), h->soft_bits.get(), h->C, tetra_soft::kFreshPrev };
    hipLaunchKernelGGL(k_reset_demod, dim3((unsigned)n), dim3(kLanes), 0, s, dv, sv, d_channels, h->C);
    HIP_TRY(h, hipGetLastError());
    if (!h->one_stream) {
        HIP_TRY(h, hipEventRecord(h->ev_reset, s));
        HIP_TRY(h, hipStreamWaitEvent(st, h->ev_reset, 0));
    }
    if (elapsed) {      // the whole tail part in one launch: the channel's own state is read before it is cleared
        hipLaunchKernelGGL(k_resume_tail, dim3((unsigned)n), dim3(kLanes), 0, st, bv, cv, lv, mv, av, d_channels, h->C, *elapsed, p->window, p->max_slots);
        HIP_TRY(h, hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_reset_tail, dim3((unsigned)n), dim3(kLanes), 0, st, bv, cv, lv, d_channels, h->C);
        HIP_TRY(h, hipGetLastError());
    }
    if (!elapsed && mv.cell_words > 0) {
        hipLaunchKernelGGL(k_reset_miss, dim3((unsigned)n), dim3(kLanes), 0, st, mv, d_channels, h->C);
        HIP_TRY(h, hipGetLastError());
    }
    if (!elapsed && av.cell_words > 0) {      // a handle that has handed over: the listed channels' hand-over fields, like the miss counters ...
        hipLaunchKernelGGL(k_reset_miss, dim3((unsigned)n), dim3(kLanes), 0, st, av, d_channels, h->C);
        HIP_TRY(h, hipGetLastError());
    }
    if (d_donors) {      // ... and behind all of it the planting
        retune::BsyncView bsv;
        TETRA_TRY(retune_impl::bsync_view(h->bs, &bsv));
        const handover::View hv = { reinterpret_cast<bsync_core::State*>(bsv.state), reinterpret_cast<bsync_core::Assist*>(av.cell),
                                          reinterpret_cast<tetra_lmac::TrackState*>(cv.cell) };
        hipLaunchKernelGGL(k_handover_plant, dim3((unsigned)((n + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, hv, d_channels, d_donors, n, h->C, p->window,
                           p->max_slots);
        HIP_TRY(h, hipGetLastError());
    }
    if (h->one_stream) HIP_TRY(h, hipEventRecord(h->ev_reset, s));
    h->reset_pending = true;
    if (h->calls > 0) {      // who waits for the last call waits for the reset too
        HIP_TRY(h, hipEventRecord(h->ev_demod[last], s));
        HIP_TRY(h, hipEventRecord(h->ev_tail[last], st));
    }
    *tail_reader = h->one_stream ? nullptr : st;
    return TETRA_OK;
}

// tetra_rx_reset_channels_device, and with donors [n] and checked parameters tetra_rx_handover_channels_device: the list travels as
// [n channels] or [n channels | n donors].  elapsed != null (and no donors): tetra_rx_resume_channels_device.
int reset_channels(tetra_rx* h, const int32_t* channels, const int32_t* donors, int n, const tetra_handover_params_t* p, void* hip_stream,
                   const uint32_t* elapsed = nullptr) {
    if (n == 0) return TETRA_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    std::vector<int32_t> both;
    void* fields = nullptr;      // the handle's first hand-over allocates them; from here on its tails run the ASSIST-capable kernels
    if (donors || elapsed) TETRA_TRY(retune_impl::bsync_assist(h->bs, &fields));
    if (donors) {
        both.assign(channels, channels + n);
        both.insert(both.end(), donors, donors + n);
    }
    int32_t* d_list = nullptr;
    hipError_t e = hipSuccess;
    const int k = donors ? h->to_device.push(both.data(), 2 * n, 2 * h->C, s, &d_list, &e) : h->to_device.push(channels, n, h->C, s, &d_list, &e);
    if (k < 0) HIP_TRY(h, e);
    hipStream_t tail = nullptr;
    TETRA_TRY(reset_enqueue(h, d_list, n, s, &tail, donors ? d_list + n : nullptr, p, elapsed));
    HIP_TRY(h, h->to_device.done(k, 0, s));
    if (tail) HIP_TRY(h, h->to_device.done(k, 1, tail));
    return TETRA_OK;
}

// The wideband receiver's retune: bins [S], and -- donors != null -- per slot a donor or -1, with checked parameters
int wbrx_retune(tetra_wbrx* h, const int32_t* bins, const int32_t* donors, const tetra_handover_params_t* p, void* hip_stream) {
    if (!h || !bins) return TETRA_ERR_ARG;
    const int S = h->n_bins;
    if (!distinct_in_range(bins, S, h->M)) return TETRA_ERR_ARG;
    std::vector<int32_t> list;               // [n slots | n bins] of the slots that move, and with donors [| n donors]
    for (int j = 0; j < S; j++)
        if (bins[j] != h->bins[(size_t)j]) list.push_back(j);
    const int n = (int)list.size();
    for (int i = 0; i < n; i++) list.push_back(bins[list[(size_t)i]]);
    for (int i = 0; donors && i < n; i++) {      // a moving slot's donor: -1, or a slot whose bin stays
        const int32_t d = donors[list[(size_t)i]];
        if (d < -1 || d >= S || (d >= 0 && bins[d] != h->bins[(size_t)d])) return TETRA_ERR_ARG;
        list.push_back(d);
    }
    if (n == 0) {
        h->retunes++;
        return TETRA_OK;
    }
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    tetra_resamp* rs = h->rs;
    tetra_rx* rx = h->rx;
    void* fields = nullptr;      // the chain's first hand-over allocates them (reset_channels)
    if (donors) TETRA_TRY(retune_impl::bsync_assist(rx->bs, &fields));
    // chan_out's rows are in the ring and the delay line is the last call's once that call's work on its stream is through
    if (h->done_recorded) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_done, 0));
    int32_t* d_list = nullptr;
    hipError_t e = hipSuccess;
    const int k = h->to_device.push(list.data(), (int)list.size(), (donors ? 3 : 2) * S, s, &d_list, &e);
    if (k < 0) HIP_TRY(h, e);
    const int hist = rs->T - 1, cells = hist * n;      // (the delay line's layout does not depend on the resampler's lane-unit width)
    hipLaunchKernelGGL(k_retune_columns, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, h->ring.get(), h->M, hist, rs->n_total, d_list, n, rs->C,
                       rs->hist.get(), h->d_bins.get());
    const hipError_t launched = hipGetLastError();
    (void)h->to_device.done(k, 0, s);
    HIP_TRY(h, launched);              // nothing has changed so far, on the device or here
    // The device's bin list and delay line move with that launch, so from here on the host state is committed whatever becomes
    // of the rest; a failure below is reported, and leaves the moved slots' chain state undefined until tetra_wbrx_reset.
    if (h->all) {      // from now on the selecting resampler, over a delay line that already holds every bin in order
        (void)retune_impl::resamp_narrow_units(rs);
        h->all = false;
    }
    for (int i = 0; i < n; i++) h->bins[(size_t)list[(size_t)i]] = list[(size_t)(n + i)];
    h->retunes++;
    h->slots_changed += n;
    hipStream_t tail = nullptr;
    int rc = reset_enqueue(rx, d_list, n, s, &tail, donors ? d_list + 2 * n : nullptr, p);
    hipError_t late = h->to_device.done(k, 0, s);
    if (late == hipSuccess && tail) late = h->to_device.done(k, 1, tail);
    if (late == hipSuccess) late = hipEventRecord(h->ev_done, s);
    if (late == hipSuccess) h->done_recorded = true;
    else if (rc == TETRA_OK) {
        h->last_hip = (int)late;
        rc = TETRA_ERR_HIP;
    }
    return rc;
}

// A stream gap of a wideband handle (include/ext/tetra_gap.h), all on the caller's stream behind the last call: the front end as
// tetra_wbrx_reset leaves it, then every slot resumed as its own heir after the bits the lost samples would have become.
int wbrx_gap(tetra_wbrx* h, int64_t n_lost, const tetra_handover_params_t* p, int64_t* elapsed_bits_out, void* hip_stream) {
    tetra_resamp* rs = h->rs;
    tetra_rx* rx = h->rx;
    const tetra_demod_config_t& dc = rx->cfg.demod;
    const double bits = std::floor((double)n_lost * (double)rs->I * 2.0 * dc.symbolrate / ((double)rs->DN * (double)h->cfg.chan.decimation * dc.samplerate) + 0.5);
    if (!(bits >= 0.0 && bits <= (double)TETRA_GAP_MAX_ELAPSED_BITS)) return TETRA_ERR_ARG;
    const uint32_t elapsed = (uint32_t)bits;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    void* fields = nullptr;      // the chain's first gap or hand-over allocates them
    TETRA_TRY(retune_impl::bsync_assist(rx->bs, &fields));
    const int S = h->n_bins;
    std::vector<int32_t> list((size_t)S);
    for (int j = 0; j < S; j++) list[(size_t)j] = j;
    if (h->done_recorded) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_done, 0));
    int32_t* d_list = nullptr;
    hipError_t e = hipSuccess;
    const int k = h->to_device.push(list.data(), S, 3 * S, s, &d_list, &e);      // (the ring's blocks at the size the retunes use)
    if (k < 0) HIP_TRY(h, e);
    // From here on the handle is committed to the gap; a failure below is reported and leaves the stream undefined until tetra_wbrx_reset.
    int rc = retune_impl::chan_restart(h->chan, s);
    hipError_t late = rs->hist.reset_on(s);
    rs->n_total = 0;
    rs->m_next = 0;
    if (late == hipSuccess) late = hipMemsetAsync(h->ring.get(), 0, h->ring.bytes(), s);
    hipStream_t tail = nullptr;
    if (rc == TETRA_OK && late == hipSuccess) rc = reset_enqueue(rx, d_list, S, s, &tail, nullptr, p, &elapsed);
    if (late == hipSuccess) late = h->to_device.done(k, 0, s);
    if (late == hipSuccess && tail) late = h->to_device.done(k, 1, tail);
    if (late == hipSuccess) late = hipEventRecord(h->ev_done, s);
    if (late == hipSuccess) h->done_recorded = true;
    else if (rc == TETRA_OK) {
        h->last_hip = (int)late;
        rc = TETRA_ERR_HIP;
    }
    if (rc == TETRA_OK && elapsed_bits_out) *elapsed_bits_out = (int64_t)elapsed;
    return rc;
}

}  // namespace

extern "C" {

int tetra_rx_reset_channels_device(tetra_rx_t* h, const int32_t* channels, int n, void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h || n < 0 || n > h->C || (!channels && n > 0)) return TETRA_ERR_ARG;
    if (h->owned) return TETRA_ERR_UNSUPPORTED;          // a wideband handle's chain: tetra_wbrx_retune restarts its slots
    if (!distinct_in_range(channels, n, h->C)) return TETRA_ERR_ARG;
    return reset_channels(h, channels, nullptr, n, nullptr, hip_stream);
}

int tetra_rx_handover_channels_device(tetra_rx_t* h, const int32_t* channels, const int32_t* donors, int n, const tetra_handover_params_t* p,
                                      void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h || n < 0 || n > h->C || ((!channels || !donors) && n > 0)) return TETRA_ERR_ARG;
    if (h->owned) return TETRA_ERR_UNSUPPORTED;          // a wideband handle's chain: tetra_wbrx_retune_from hands its slots over
    tetra_handover_params_t prm;
    if (!distinct_in_range(channels, n, h->C) || !handover_params(p, &prm)) return TETRA_ERR_ARG;
    std::vector<char> heir((size_t)h->C, 0);
    for (int i = 0; i < n; i++) heir[(size_t)channels[i]] = 1;
    for (int i = 0; i < n; i++)
        if (donors[i] < -1 || donors[i] >= h->C || (donors[i] >= 0 && heir[(size_t)donors[i]])) return TETRA_ERR_ARG;
    return reset_channels(h, channels, donors, n, &prm, hip_stream);
}

int tetra_rx_resume_channels_device(tetra_rx_t* h, const int32_t* channels, int n, int64_t elapsed_bits, const tetra_handover_params_t* p,
                                    void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h || n < 0 || n > h->C || (!channels && n > 0)) return TETRA_ERR_ARG;
    if (h->owned) return TETRA_ERR_UNSUPPORTED;          // a wideband handle's chain: tetra_wbrx_gap resumes its slots
    tetra_handover_params_t prm;
    if (!distinct_in_range(channels, n, h->C) || !gap_params(p, &prm) || elapsed_bits < 0 || elapsed_bits > TETRA_GAP_MAX_ELAPSED_BITS) return TETRA_ERR_ARG;
    const uint32_t elapsed = (uint32_t)elapsed_bits;
    return reset_channels(h, channels, nullptr, n, &prm, hip_stream, &elapsed);
}

int tetra_wbrx_gap(tetra_wbrx_t* h, int64_t n_lost, const tetra_handover_params_t* p, int64_t* elapsed_bits_out, void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    tetra_handover_params_t prm;
    if (!h || n_lost < 0 || !gap_params(p, &prm)) return TETRA_ERR_ARG;
    return wbrx_gap(h, n_lost, &prm, elapsed_bits_out, hip_stream);
}

int tetra_wbrx_retune(tetra_wbrx_t* h, const int32_t* bins, void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    return wbrx_retune(h, bins, nullptr, nullptr, hip_stream);
}

int tetra_wbrx_retune_from(tetra_wbrx_t* h, const int32_t* bins, const int32_t* donors, const tetra_handover_params_t* p, void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    tetra_handover_params_t prm;
    if (!handover_params(p, &prm)) return TETRA_ERR_ARG;
    return wbrx_retune(h, bins, donors, &prm, hip_stream);
}

int tetra_wbrx_retune_count(tetra_wbrx_t* h, int64_t* retunes, int64_t* slots_changed) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h) return TETRA_ERR_ARG;
    if (retunes) *retunes = h->retunes;
    if (slots_changed) *slots_changed = h->slots_changed;
    return TETRA_OK;
}

}  // extern "C"
