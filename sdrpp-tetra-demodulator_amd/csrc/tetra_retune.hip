// tetra_retune.hip -- retuning while the stream runs (include/tetra_retune.h): the stream-ordered reset of listed channels of the
// receive chain, and the wideband receiver's retune of carrier slots on top of it.
//
// Nothing here waits on the host.  Two calls may be in flight (the demodulator of call k + 1 runs beside the tail of call k), so a
// reset between call k and call k + 1 is split by stream:
//
//   caller's stream  [wait: demodulator k]  (wideband: bin list, delay-line columns)  k_reset_demod           (event ev_reset)
//   tail stream      [behind tail k, wait ev_reset]  k_restart_tail: the tail's per-channel tables, and the planting
//
// and call k + 1 is ordered behind both: its demodulator waits for ev_reset, its tail runs on the tail stream.  The events of call k
// (ev_demod, ev_tail, the wideband ev_done) are recorded again behind the reset, so whoever waits for that call -- tetra_rx_wait,
// the state readers, the call after next -- also waits for the reset.  Call k's results are not touched: they stay fetchable.
//
// The kernels are a launch of one 64-lane workgroup per listed channel (lane code: retune_core.hpp): not a hot path.
// A reset with donors (include/ext/tetra_handover.h) and a stream gap (include/ext/tetra_gap.h) are the same two launches: k_restart_tail
// reads the anchor of the channel's source -- its donor as the last tail left it, or the channel itself -- before it clears the channel,
// and plants behind the clearing (lane code: handover_core.hpp).  The wideband handle's gap puts the front end's restart in front, on
// the caller's stream: what tetra_wbrx_reset leaves, without its host synchronisation.
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

// The tail part of every restart -- plain reset, hand-over, stream gap -- of listed channel c: the anchor of its source is read, then
// all lanes clear the tail's tables of c (retune_core.hpp: reset_tail_channel), then lane 0 plants (handover_core.hpp).  The source is
// c itself (own), donors[i], or none: a plain reset (donors null) or a hand-over entry with donor -1, where nothing is planted and the
// hand-over fields stay zero (status NONE).  A donor is never an heir -- the host has checked it --, so no workgroup clears what
// another reads; a channel that is its own source is read and cleared by one workgroup, the barrier between.
__global__ __launch_bounds__(kLanes) void k_restart_tail(retune::TailView t, const int32_t* __restrict__ channels, const int32_t* __restrict__ donors, int own,
                                                         int n_channels, uint32_t elapsed, int32_t window, int32_t max_slots) {
    const int c = channels[blockIdx.x];
    if (c < 0 || c >= n_channels) return;          // (the host has checked the lists)
    int src = own ? c : donors ? donors[blockIdx.x] : -1;
    if (src >= n_channels) src = -1;
    const handover::View v = handover::view_of(t);
    handover::Anchor an = {};
    if (src >= 0) an = handover::anchor_of(v, src, own != 0);
    __syncthreads();
    retune::reset_tail_channel(t, c, threadIdx.x, kLanes);
    __syncthreads();
    if (src >= 0 && threadIdx.x == 0) handover::plant(v, c, an, elapsed, window, max_slots);
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

// What the listed channels restart from, made by one of the three functions: a plain reset, a hand-over (per listed channel its donor
// or -1, with checked parameters), or a stream gap of `elapsed` bits in which every listed channel is its own heir.
struct Restart {
    enum Kind { kPlain, kFromDonors, kOwnHeir } kind;
    const int32_t* donors;               // kFromDonors: [n], the caller's list on the way in, the device's at the launch
    tetra_handover_params_t p;           // kFromDonors, kOwnHeir
    uint32_t elapsed;                    // kOwnHeir
    static Restart plain() { return { kPlain, nullptr, { 0, 0 }, 0u }; }
    static Restart from_donors(const int32_t* donors, const tetra_handover_params_t& p) { return { kFromDonors, donors, p, 0u }; }
    static Restart own_heir(const tetra_handover_params_t& p, uint32_t elapsed) { return { kOwnHeir, nullptr, p, elapsed }; }
    bool plants() const { return kind != kPlain; }
};

// The chain's part, for n > 0 channels listed on the device at d_channels (uploaded on s; r.donors on the device too).  The caller marks
// the list's readers: s, and *tail_reader (the tail stream when the chain has one of its own, else null).
int reset_enqueue(tetra_rx* h, const int32_t* d_channels, int n, hipStream_t s, hipStream_t* tail_reader, const Restart& r) {
    retune::DemodView dv;
    retune::BsyncView bv;
    TETRA_TRY(retune_impl::demod_view(h->dem, &dv));
    TETRA_TRY(retune_impl::bsync_view(h->bs, &bv));
    static_assert(sizeof(tetra_lmac_cell_state_t) % 4 == 0 && sizeof(tetra_rx_link_t) % 4 == 0, "reset in 32-bit words");
    // the chain's per-channel tables in 32-bit words per channel: no words where the handle has no such table, nor for miss counters
    // that the rule in force does not count
    retune::CellView tab[kChanTablesAll];
    for (int t = 0; t < kChanTablesAll; ++t) {
        void* at = nullptr;
        bool counting = true;
        TETRA_TRY(chan_tab::live(h, t, &at, &counting));
        tab[t] = { static_cast<uint32_t*>(at), at && counting ? (int32_t)(chan_tab::elem_bytes(t) / 4) : 0 };
    }
    const retune::TailView tv = { bv, tab[TAB_CELL], tab[TAB_LINK], tab[TAB_SYNC_MISSES], tab[TAB_HANDOVER] };
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
    hipLaunchKernelGGL(k_restart_tail, dim3((unsigned)n), dim3(kLanes), 0, st, tv, d_channels, r.donors, r.kind == Restart::kOwnHeir ? 1 : 0, h->C, r.elapsed,
                       r.p.window, r.p.max_slots);
    HIP_TRY(h, hipGetLastError());
    if (h->one_stream) HIP_TRY(h, hipEventRecord(h->ev_reset, s));
    h->reset_pending = true;
    if (h->calls > 0) {      // who waits for the last call waits for the reset too
        HIP_TRY(h, hipEventRecord(h->ev_demod[last], s));
        HIP_TRY(h, hipEventRecord(h->ev_tail[last], st));
    }
    *tail_reader = h->one_stream ? nullptr : st;
    return TETRA_OK;
}

// The three tetra_rx_*_channels_device entries behind their argument checks: the list travels as [n channels], with donors as
// [n channels | n donors].
int reset_channels(tetra_rx* h, const int32_t* channels, int n, const Restart& r, void* hip_stream) {
    if (n == 0) return TETRA_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    std::vector<int32_t> list(channels, channels + n);
    void* fields = nullptr;      // the handle's first hand-over or gap allocates them; from here on its tails run the ASSIST-capable kernels
    if (r.plants()) TETRA_TRY(retune_impl::bsync_assist(h->bs, &fields));
    if (r.donors) list.insert(list.end(), r.donors, r.donors + n);
    int32_t* d_list = nullptr;
    hipError_t e = hipSuccess;
    const int k = h->to_device.push(list.data(), (int)list.size(), (r.donors ? 2 : 1) * h->C, s, &d_list, &e);
    if (k < 0) HIP_TRY(h, e);
    Restart on_device = r;
    if (r.donors) on_device.donors = d_list + n;
    hipStream_t tail = nullptr;
    TETRA_TRY(reset_enqueue(h, d_list, n, s, &tail, on_device));
    HIP_TRY(h, h->to_device.done(k, 0, s));
    if (tail) HIP_TRY(h, h->to_device.done(k, 1, tail));
    return TETRA_OK;
}

// What the three tetra_rx_*_channels_device entries check alike, in their order; lists_given: every list the entry takes is non-null
int channel_list_status(const tetra_rx* h, const int32_t* channels, int n, bool lists_given) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h || n < 0 || n > h->C || (!lists_given && n > 0)) return TETRA_ERR_ARG;
    if (h->owned) return TETRA_ERR_UNSUPPORTED;          // a wideband handle's chain: tetra_wbrx_retune, _retune_from and _gap restart its slots
    return distinct_in_range(channels, n, h->C) ? TETRA_OK : TETRA_ERR_ARG;
}

// The end that tetra_wbrx_retune and tetra_wbrx_gap share, behind the point from which the host state is committed: the chain's
// restart of the n slots listed at d_list (unless rc or late says that the front end's part has failed already), the readers of block k
// of the upload ring marked, ev_done recorded behind it all, and a late HIP error folded into the return code.
int wbrx_commit(tetra_wbrx* h, int k, const int32_t* d_list, int n, hipStream_t s, const Restart& r, int rc, hipError_t late) {
    hipStream_t tail = nullptr;
    if (rc == TETRA_OK && late == hipSuccess) rc = reset_enqueue(h->rx, d_list, n, s, &tail, r);
    if (late == hipSuccess) late = h->to_device.done(k, 0, s);
    if (late == hipSuccess && tail) late = h->to_device.done(k, 1, tail);
    if (late == hipSuccess) late = hipEventRecord(h->ev_done, s);
    if (late == hipSuccess) h->done_recorded = true;
    else if (rc == TETRA_OK) {
        h->last_hip = (int)late;
        rc = TETRA_ERR_HIP;
    }
    return rc;
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
    return wbrx_commit(h, k, d_list, n, s, donors ? Restart::from_donors(d_list + 2 * n, *p) : Restart::plain(), TETRA_OK, hipSuccess);
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
    rc = wbrx_commit(h, k, d_list, S, s, Restart::own_heir(*p, elapsed), rc, late);
    if (rc == TETRA_OK && elapsed_bits_out) *elapsed_bits_out = (int64_t)elapsed;
    return rc;
}

}  // namespace

extern "C" {

int tetra_rx_reset_channels_device(tetra_rx_t* h, const int32_t* channels, int n, void* hip_stream) {
    const int rc = channel_list_status(h, channels, n, channels != nullptr);
    return rc != TETRA_OK ? rc : reset_channels(h, channels, n, Restart::plain(), hip_stream);
}

int tetra_rx_handover_channels_device(tetra_rx_t* h, const int32_t* channels, const int32_t* donors, int n, const tetra_handover_params_t* p,
                                      void* hip_stream) {
    const int rc = channel_list_status(h, channels, n, channels && donors);
    if (rc != TETRA_OK) return rc;
    tetra_handover_params_t prm;
    if (!handover_params(p, &prm)) return TETRA_ERR_ARG;
    std::vector<char> heir((size_t)h->C, 0);
    for (int i = 0; i < n; i++) heir[(size_t)channels[i]] = 1;
    for (int i = 0; i < n; i++)      // a donor is never an heir: k_restart_tail relies on it
        if (donors[i] < -1 || donors[i] >= h->C || (donors[i] >= 0 && heir[(size_t)donors[i]])) return TETRA_ERR_ARG;
    return reset_channels(h, channels, n, Restart::from_donors(donors, prm), hip_stream);
}

int tetra_rx_resume_channels_device(tetra_rx_t* h, const int32_t* channels, int n, int64_t elapsed_bits, const tetra_handover_params_t* p,
                                    void* hip_stream) {
    const int rc = channel_list_status(h, channels, n, channels != nullptr);
    if (rc != TETRA_OK) return rc;
    tetra_handover_params_t prm;
    if (!gap_params(p, &prm) || elapsed_bits < 0 || elapsed_bits > TETRA_GAP_MAX_ELAPSED_BITS) return TETRA_ERR_ARG;
    return reset_channels(h, channels, n, Restart::own_heir(prm, (uint32_t)elapsed_bits), hip_stream);
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
