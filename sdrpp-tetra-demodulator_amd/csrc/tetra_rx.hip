// tetra_rx.hip -- the device-resident receive chain behind one handle (include/tetra_rx.h): the ordering, buffers, streams and
// events around this library's own stage entry points.
//
// Reference chain per receiver: tetra_burst_sync_in (phy/tetra_burst_sync.c:54-155) -> tetra_burst_rx_cb (phy/tetra_burst.c:343-393)
// -> tp_sap_udata_ind (lower_mac/tetra_lower_mac.c:148-237) with the cell state fed back at :246-275.  Here, per process call k:
//
//   caller's stream  [wait: tail k-2 has read bit rows k & 1]  demodulator -> bits[k & 1]                          (event D_k)
//   tail stream      [wait D_k]  synchroniser (packed frames, types, bit numbers, counts)
//                    frame lists (SYNC / NORM_1 / NORM_2 / any) in one pass
//                    SB1:   decode straight from the SYNC frames -> tracker: cell state, per-slot scrambling code, TDMA time
//                           before / after the slot's SB1, the SB1 rows' labels
//                    every other configured kind: ONE launch that decodes them all straight from the frames with the TRACKER's
//                           per-slot codes and labels every row (channel, slot, bit number, times, crc)            (event T_k)
//
// so the demodulator of call k+1 runs beside the tail of call k; results and bit rows are double buffered by call parity.
// With TETRA_RX_FLAG_SOFT the demodulator also writes its symbols, k_soft (below) follows it on the caller's stream in front of D_k and
// leaves the call's soft values in the channels' rings, and the tail decodes SB1 and the other coded kinds from those rings
// (lmac_impl::decode_frames with the ring among its options) with the AACH in a launch of its own: 9 launches (soft_core.hpp).
// Every option of the decoder -- soft values, bit-error counts, ranks -- reaches it as one lmac_impl::FrameOpts built from the handle's flags.
// (Until round 6: per kind a compacting demultiplexer into byte rows (4 launches), a counted decode and a label kernel -- 40 launches
// and 0.36 GB of byte rows per second of 4096 channels; now 7 launches and no byte rows.)
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/tetra_aach.h"
#include "../../include/ext/tetra_aach_soft.h"
#include "../../include/ext/tetra_biterr.h"
#include "../../include/ext/tetra_handover.h"
#include "../../include/ext/tetra_list.h"
#include "../../include/ext/tetra_sync_tol.h"
#include "../../include/tetra_rx.h"
#include "handover_core.hpp"
#include "lmac_impl.hpp"
#include "rx_handle.hpp"
#include "rx_out_core.hpp"
#include "soft_core.hpp"

namespace {

// TETRA_RX_FLAG_SOFT: the call's symbols -> soft values in the channels' rings (soft_core.hpp), a thread per symbol.  A channel's
// carried state (previous symbol, absolute bit count) is read at `in` and written at `out`, the other parity: one launch, and no
// workgroup reads what another one writes.  The demodulator delivers whole symbols, so a channel's bit count is even and a symbol's two
// soft values are one aligned 2-byte store.
__global__ __launch_bounds__(256) void k_soft(const float2* __restrict__ sym, int sym_stride, const int32_t* __restrict__ n_bits,
                                              const float2* __restrict__ prev_in, const uint32_t* __restrict__ bits_in, float2* __restrict__ prev_out,
                                              uint32_t* __restrict__ bits_out, int8_t* __restrict__ ring, uint32_t ring_size) {
    const int c = blockIdx.y, k = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const float2* z = sym + (size_t)c * sym_stride;
    const int n = min(max(n_bits[c] >> 1, 0), sym_stride);
    const uint32_t count = bits_in[c];
    const float2 pv = prev_in[c];
    if (k == 0) {
        bits_out[c] = count + 2u * (uint32_t)n;
        prev_out[c] = n > 0 ? z[n - 1] : pv;
    }
    if (k >= n) return;
    const float2 s = z[k], p = k > 0 ? z[k - 1] : pv;
    int q0, q1;
    tetra_soft::soft_pair(s.x, s.y, p.x, p.y, q0, q1);
    const uint32_t at = (count + 2u * (uint32_t)k) & (ring_size - 1u) & ~1u;
    *reinterpret_cast<uint16_t*>(ring + (size_t)c * ring_size + at) = (uint16_t)((q0 & 0xff) | ((q1 & 0xff) << 8));
}

// the type-1 bits of the first n rows, packed: out[j][0 .. nb) = t2[j][0 .. nb) (two bytes per thread: every kind's count is even)
__global__ __launch_bounds__(256) void k_rx_pack_type1(const uint8_t* __restrict__ t2, int in_stride, int nb, int n, uint8_t* __restrict__ out) {
    const int half = nb >> 1;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * half) return;
    const int j = (int)(i / half), u = (int)(i - (long long)j * half);
    reinterpret_cast<uint16_t*>(out)[i] = reinterpret_cast<const uint16_t*>(t2 + (size_t)j * in_stride)[u];
}

// byte `at` of the first n rows, packed (fetch_col: a column that lies inside the rows)
__global__ __launch_bounds__(256) void k_rx_pack_byte(const uint8_t* __restrict__ t2, int in_stride, int at, int n, uint8_t* __restrict__ out) {
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j < n) out[j] = t2[(size_t)j * in_stride + at];
}

// TETRA_RX_FLAG_BITERR: a call's coded rows into the channels' link figures (tetra_rx_link_t).  The rows of a kind are in (channel, frame)
// order and chan_first says where a channel's begin in each frame list, so a wavefront takes one channel, walks its rows of every coded
// kind, reduces across its lanes and adds to the channel's figures: no two wavefronts share a channel and tails run one after the other,
// so plain stores do.
struct LinkKind {
    const int32_t* ok;            // the kind's verdicts and counts, per row
    const uint32_t* biterr;
    int list;                     // the frame list its rows come from
};
struct LinkTable {
    LinkKind kind[TETRA_RX_N_KINDS];
    int n;
};
__global__ __launch_bounds__(64) void k_rx_link(const LinkTable tab, const int32_t* __restrict__ chan_first, const int32_t* __restrict__ counts, int C,
                                                tetra_rx_link_t* __restrict__ link) {
    const int c = blockIdx.x, lane = threadIdx.x;
    uint32_t bits = 0, errors = 0, blocks = 0, bad = 0;          // (a call's share of one channel: far below 2^32)
    for (int k = 0; k < tab.n; ++k) {
        const LinkKind K = tab.kind[k];
        const int first = chan_first[(size_t)K.list * C + c];
        const int end = c + 1 < C ? chan_first[(size_t)K.list * C + c + 1] : counts[K.list];
        for (int j = first + lane; j < end; j += 64) {
            const bool good = K.ok[j] != 0;
            const uint32_t v = K.biterr[j];
            blocks += 1u;
            bad += good ? 0u : 1u;
            bits += good ? v >> 16 : 0u;
            errors += good ? v & 0xffffu : 0u;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bits += (uint32_t)__shfl_xor((int)bits, d);
        errors += (uint32_t)__shfl_xor((int)errors, d);
        blocks += (uint32_t)__shfl_xor((int)blocks, d);
        bad += (uint32_t)__shfl_xor((int)bad, d);
    }
    if (lane == 0) {
        tetra_rx_link_t l = link[c];
        l.bits += bits;
        l.bit_errors += errors;
        l.blocks += blocks;
        l.blocks_crc_bad += bad;
        link[c] = l;
    }
}

// tetra_rx_out_set_snapshot (ext/tetra_rx_out_ext.h): the armed per-channel tables as this tail leaves them -> the parity's snapshot, in
// 32-bit words (every table's element is a whole number of them), a thread per word of the longest table.  Reads what earlier kernels
// of the tail wrote; nothing in the tail reads what it writes.
struct SnapTable {
    const uint32_t* src;
    uint32_t* dst;
    int words;                    // 0: not armed
};
struct SnapArgs {
    SnapTable tab[rx_out::kChanTables];
};
__global__ __launch_bounds__(256) void k_rx_snapshot(const SnapArgs a) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
#pragma unroll
    for (int t = 0; t < rx_out::kChanTables; ++t)
        if (i < a.tab[t].words) a.tab[t].dst[i] = a.tab[t].src[i];
}

// The hand-over's apply step (include/ext/tetra_handover.h; lane code: handover_core.hpp) between the synchroniser and the tracker, a
// thread per channel: the synchroniser's result word advances the channel's PHY time or zeroes its cell.  Only on a handle that has
// ever handed over.
__global__ __launch_bounds__(64) void k_handover_apply(handover::View v, int n_channels) {
    const int c = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (c < n_channels) handover::apply_channel(v, c);
}

template <typename T> bool dalloc(DevMem<T>& p, size_t count) { return p.reserve(sizeof(T) * (count ? count : 1)) == hipSuccess; }

int zero_results(tetra_rx* h) {
    for (int b = 0; b < 2; b++) HIP_TRY(h, hipMemset(h->counts[b], 0, sizeof(int32_t) * TETRA_N_LISTS));
    for (int t = 0; t < rx_out::kChanTables; ++t) {      // the chain's own tables (tetra_bsync_reset clears the synchroniser's)
        void* p = nullptr;
        if (chan_tab::own(t) && chan_tab::live(h, t, &p) == TETRA_OK && p) HIP_TRY(h, hipMemset(p, 0, (size_t)rx_out::chan_elem_bytes(t) * (size_t)h->C));
    }
    for (int b = 0; b < 2; b++) HIP_TRY(h, hipMemset(h->nbits[b], 0, sizeof(int32_t) * (size_t)h->C));
    if (h->soft) {      // fresh channels: previous symbol (1,1)/sqrt(2), bit count 0 (both parities: the next call reads either)
        const std::vector<float> prev((size_t)4 * h->C, tetra_soft::kFreshPrev);
        HIP_TRY(h, hipMemcpy(h->soft_prev, prev.data(), sizeof(float) * prev.size(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemset(h->soft_bits, 0, sizeof(uint32_t) * 2 * (size_t)h->C));
    }
    return TETRA_OK;
}

// the tail of one call on stream s (see the header of this file)
int enqueue_tail(tetra_rx* h, int b, hipStream_t s) {
    const int n = h->rows;
    HIP_TRY(h, hipEventRecord(h->ev_stage[0], s));
    TETRA_TRY(tetra_bsync_process_packed_device(h->bs, h->bits[b], h->stride, h->nbits[b], h->frames, h->ft, h->fb, h->nf, s));
    HIP_TRY(h, hipEventRecord(h->ev_stage[1], s));
    TETRA_TRY(tetra_burst_index_device(h->ft, n, h->F, h->lists[b], h->counts[b], h->chan_first, h->index_work, s));
    void* assist = nullptr;
    TETRA_TRY(chan_tab::live(h, TAB_HANDOVER, &assist));
    if (assist) {      // a handle that has handed over: the synchroniser's results of this call, in front of the tracker
        const handover::View hv = { nullptr, static_cast<bsync_core::Assist*>(assist), reinterpret_cast<tetra_lmac::TrackState*>(h->cell.get()) };
        hipLaunchKernelGGL(k_handover_apply, dim3((unsigned)((h->C + 63) / 64)), dim3(64), 0, s, hv, h->C);
        HIP_TRY(h, hipGetLastError());
    }
    tetra_lmac_frames_t src = {};
    src.d_frames = h->frames;
    src.d_frame_type = h->ft;
    src.n_frames = n;
    src.frames_per_channel = h->F;
    src.d_frame_bitnum = h->fb;
    src.d_time_rx = h->row_time_rx;
    src.d_time = h->row_time;
    src.d_workspace = h->lmac_ws;
    src.workspace_bytes = h->lmac_ws.bytes();
    // the handle's flags as the decoder's options, once: without a flag its array is NULL and the launches are the ones they were
    const lmac_impl::SoftRing ring = { h->soft_ring, h->soft_R };
    uint32_t* counts[TETRA_RX_N_KINDS];          // per job where its bit-error counts go (NULL: the AACH)
    int32_t* ranks[TETRA_RX_N_KINDS];            // ... and its ranks (NULL: the AACH)
    lmac_impl::FrameOpts opts;
    opts.soft = h->soft ? &ring : nullptr;
    opts.d_biterr = h->biterr ? counts : nullptr;
    opts.d_rank = h->list ? ranks : nullptr;
    opts.max_candidates = h->list_T;
    opts.list_work.d_work = h->list_ws;          // the list launches' compaction words (one launch at a time on this stream)
    opts.list_work.bytes = h->list_ws.bytes();
    auto job_of = [&](int k, bool labels) {
        const KindInfo& ki = kKinds[k];
        const KindBufs& r = h->res[b][k];
        tetra_lmac_job_t j = {};
        j.type = ki.tpsap | (k == TETRA_RX_KIND_BBK && h->aach_rm ? TETRA_LMAC_JOB_RM3014 : 0);
        if (k == TETRA_RX_KIND_BBK && h->aach_soft) j.type |= TETRA_LMAC_JOB_RM3014_SOFT | TETRA_LMAC_JOB_AACH_MIN_MARGIN(h->aach_min_margin);
        j.blk_num = ki.blk;
        j.d_row_frame = r.row_frame;
        j.d_n_rows = r.n_rows;
        j.max_rows = n;
        j.out_stride = ki.out_stride;
        j.d_frame_scramb = h->row_scramb;
        j.d_type2 = r.t2;
        j.d_crc_ok = r.ok;
        j.d_labels = labels ? reinterpret_cast<tetra_lmac_label_t*>(r.blocks.get()) : nullptr;
        return j;
    };
    {   // SB1 first: its SYNC PDUs set the code and the clock for everything else in the same burst (tetra_lower_mac.c:246-275)
        const KindBufs& r = h->res[b][TETRA_RX_KIND_SB1];
        const tetra_lmac_job_t j = job_of(TETRA_RX_KIND_SB1, false);
        counts[0] = r.biterr;
        ranks[0] = r.rank;
        TETRA_TRY(lmac_impl::decode_frames(&src, &j, 1, opts, s));      // (with ranks the rescue runs in front of the tracker: a rescued SYNC PDU sets code and clock)
        TETRA_TRY(tetra_lmac_track_sync_lists_device(r.t2, kKinds[TETRA_RX_KIND_SB1].out_stride, r.ok, h->ft, h->nf,
                                                 h->chan_first + (size_t)TETRA_LIST_SYNC * h->C, h->C, h->F, h->cell, h->row_scramb, h->row_time_rx,
                                                 h->row_time, h->fb, reinterpret_cast<tetra_lmac_label_t*>(r.blocks.get()), s));
    }
    HIP_TRY(h, hipEventRecord(h->ev_stage[2], s));
    tetra_lmac_job_t jobs[TETRA_RX_N_KINDS];
    int nj = 0;
    for (int k : kJobOrder)
        if ((h->kinds & (1 << k)) && !(h->soft && k == TETRA_RX_KIND_BBK)) {
            counts[nj] = h->res[b][k].biterr;
            ranks[nj] = h->res[b][k].rank;
            jobs[nj++] = job_of(k, true);
        }
    if (h->soft) {      // the coded kinds from the ring; the AACH in a launch of its own: from the packed frames as ever, or -- TETRA_RX_FLAG_AACH_SOFT -- from the ring too
        TETRA_TRY(lmac_impl::decode_frames(&src, jobs, nj, opts, s));
        if (!h->aach_soft) opts.soft = nullptr;
        nj = 0;
        if (h->kinds & (1 << TETRA_RX_KIND_BBK)) {
            counts[nj] = nullptr;
            ranks[nj] = nullptr;
            jobs[nj++] = job_of(TETRA_RX_KIND_BBK, true);
        }
    }
    // (the rescue of these kinds runs inside the call, behind its decode launch: in front of the link figures and of the tail's event)
    TETRA_TRY(lmac_impl::decode_frames(&src, jobs, nj, opts, s));
    if (h->biterr) {
        LinkTable tab = {};
        for (int k = 0; k < TETRA_RX_N_KINDS; ++k)
            if ((h->kinds & (1 << k)) && k != TETRA_RX_KIND_BBK) tab.kind[tab.n++] = LinkKind{ h->res[b][k].ok, h->res[b][k].biterr, kKinds[k].list };
        hipLaunchKernelGGL(k_rx_link, dim3((unsigned)h->C), dim3(64), 0, s, tab, h->chan_first.get(), h->counts[b].get(), h->C, h->link.get());
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(h->ev_stage[3], s));
    if (h->traffic) TETRA_TRY(traffic_impl::enqueue(h, b, s));      // ext/tetra_traffic.h: outside the stages' spans, in front of the tail's event
    h->snap_taken[b] = 0;
    if (h->snap_mask) {      // behind the link figures and outside the stages' spans; in front of the tail's event, which a delivery waits for
        SnapArgs a = {};
        int most = 0;
        for (int t = 0; t < rx_out::kChanTables; ++t) {
            void* src = nullptr;
            TETRA_TRY(chan_tab::live(h, t, &src));
            if (!(h->snap_mask & rx_out::chan_extra(t)) || !src) continue;
            a.tab[t].src = static_cast<const uint32_t*>(src);
            a.tab[t].dst = reinterpret_cast<uint32_t*>(h->snap[b].get() + rx_out::snap_offset(t, h->C));
            a.tab[t].words = rx_out::chan_elem_bytes(t) / 4 * h->C;
            most = a.tab[t].words > most ? a.tab[t].words : most;
            h->snap_taken[b] |= rx_out::chan_extra(t);
        }
        if (most > 0) {
            hipLaunchKernelGGL(k_rx_snapshot, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, s, a);
            HIP_TRY(h, hipGetLastError());
        }
    }
    return TETRA_OK;
}

// parity of the call `which` calls back (0 = latest); -1 if there is no such call yet
int parity_of(const tetra_rx* h, int which) {
    if (which < 0 || which > 1 || h->calls <= which) return -1;
    return (int)((h->calls - 1 - which) & 1);
}

// The rows of `kind` of call `which` are ready: what every fetch does once its arguments are checked.  No such call yet: no rows,
// TETRA_OK.  Else waits for that call's tail, reads and bounds the row count into *n_rows, and applies the capacity rule: more rows than
// `capacity` is TETRA_ERR_SIZE only if the caller `wants` them (it handed in an output pointer), TETRA_OK for one who only counts.
// copy(r, n) then brings n > 0 wanted rows over, with the handle's device still selected, and its status is the fetch's.
template <class Copy>
int fetch_rows(tetra_rx* h, int which, int kind, bool wants, int capacity, int* n_rows, Copy copy) {
    *n_rows = 0;
    const int b = parity_of(h, which);
    if (b < 0) return TETRA_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipEventSynchronize(h->ev_tail[b]));
    const KindBufs& r = h->res[b][kind];
    int32_t n = 0;
    HIP_TRY(h, hipMemcpy(&n, r.n_rows, sizeof(n), hipMemcpyDeviceToHost));
    if (n < 0 || n > h->rows) return TETRA_ERR_HIP;          // (cannot happen: the demultiplexer counts at most `rows` frames)
    *n_rows = n;
    if (n > capacity) return wants ? TETRA_ERR_SIZE : TETRA_OK;
    return n && wants ? copy(r, (int)n) : TETRA_OK;
}

// the latest call's tail is done: what the getters of per-channel state wait for
int latest_tail_done(tetra_rx* h) {
    if (h->calls > 0) HIP_TRY(h, hipEventSynchronize(h->ev_tail[(h->calls - 1) & 1]));
    return TETRA_OK;
}

// Rows that are not contiguous on the device: pack(stage) launches the kernel that packs them on the fetch stream, then ONE copy (a strided
// device-to-host copy of 10^5 narrow rows moves ~50 MB/s: 1.9 s for a second of 4096 channels' blocks, measured; this way the link's rate)
template <class Pack> int fetch_packed(tetra_rx* h, void* out, size_t bytes, Pack pack) {
    if (h->fetch_stage.reserve((size_t)h->rows * 268) != hipSuccess) {
        (void)hipGetLastError();
        return TETRA_ERR_NOMEM;
    }
    pack(h->fetch_stage.get());
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, h->fetch_stage, bytes, hipMemcpyDeviceToHost, h->fetch_s));
    HIP_TRY(h, hipStreamSynchronize(h->fetch_s));
    return TETRA_OK;
}

// The blocking fetch of one row column (COL_*; tetra_biterr.h, tetra_list.h, tetra_aach.h): a column with a buffer of its own is one
// copy, one that lies inside the rows (a byte wide) goes through fetch_packed.
int fetch_col(tetra_rx* h, int which, int kind, int col, void* out, int capacity, int* n_rows) {
    if (!h || !n_rows || kind < 0 || kind >= TETRA_RX_N_KINDS || which < 0 || which > 1 || capacity < 0) return TETRA_ERR_ARG;
    TETRA_TRY(row_col::status(h, col, kind));
    return fetch_rows(h, which, kind, out != nullptr, capacity, n_rows, [&](const KindBufs&, int n) -> int {
        const ColSrc c = row_col::src(h, parity_of(h, which), kind, col);
        const size_t elem = (size_t)rx_out::row_elem_bytes(col);
        if (c.stride == elem) {
            HIP_TRY(h, hipMemcpy(out, c.base, elem * (size_t)n, hipMemcpyDeviceToHost));
            return TETRA_OK;
        }
        return fetch_packed(h, out, (size_t)n, [&](uint8_t* stage) {
            hipLaunchKernelGGL(k_rx_pack_byte, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->fetch_s, c.base, (int)c.stride, 0, n, stage);
        });
    });
}

// ... and the same column where it is: *d_col [rows] beside tetra_rx_rows_device's rows, hip_stream made to wait for the call's tail
template <class T> int col_device(tetra_rx* h, int which, int kind, int col, const T** d_col, void* hip_stream) {
    if (!h || !d_col || kind < 0 || kind >= TETRA_RX_N_KINDS || which < 0 || which > 1) return TETRA_ERR_ARG;
    TETRA_TRY(row_col::status(h, col, kind));
    const int b = parity_of(h, which);
    if (b < 0) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), h->ev_tail[b], 0));
    *d_col = reinterpret_cast<const T*>(row_col::src(h, b, kind, col).base);
    return TETRA_OK;
}

// The getter of one per-channel table (TAB_*): channels [first, first + count) behind the latest call's tail.  The chain's own tables
// are copied from where they live; the synchroniser's are answered by its getters, which wait for the whole device and answer zeros
// for miss counters that were never allocated.
int get_chan(tetra_rx* h, int tab, int first, int count, void* out) {
    if (!h || !out || first < 0 || count < 0 || first + (long long)count > h->C) return TETRA_ERR_ARG;
    if (chan_tab::own(tab)) TETRA_TRY(chan_tab::status(h, tab));
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    TETRA_TRY(latest_tail_done(h));
    if (!count) return TETRA_OK;
    if (tab == TAB_SYNC_STATE) return tetra_bsync_get_state(h->bs, first, count, static_cast<tetra_bsync_state_t*>(out));
    if (tab == TAB_SYNC_MISSES) return tetra_bsync_get_misses(h->bs, first, count, static_cast<int32_t*>(out));
    void* live = nullptr;
    TETRA_TRY(chan_tab::live(h, tab, &live));
    const size_t elem = (size_t)rx_out::chan_elem_bytes(tab);
    HIP_TRY(h, hipMemcpy(out, static_cast<const uint8_t*>(live) + elem * (size_t)first, elem * (size_t)count, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

}  // namespace

extern "C" {

int tetra_rx_default_config(tetra_rx_config_t* cfg) {
    if (!cfg) return TETRA_ERR_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    return tetra_demod_default_config(&cfg->demod);
}

int tetra_rx_type1_bits(int kind) {
    return kind < 0 || kind >= TETRA_RX_N_KINDS ? TETRA_ERR_ARG : kKinds[kind].type1_bits;
}

int tetra_rx_create(const tetra_rx_config_t* cfg, tetra_rx_t** out) {
    if (!cfg || !out) return TETRA_ERR_ARG;
    *out = nullptr;
    if ((cfg->kinds & ~((1 << TETRA_RX_N_KINDS) - 1)) || (cfg->flags & ~(TETRA_RX_FLAG_ONE_STREAM | TETRA_RX_FLAG_AACH_RM3014 | TETRA_RX_FLAG_SOFT | TETRA_RX_FLAG_BITERR | TETRA_RX_FLAG_SYNC_TOLERANT | TETRA_RX_FLAG_LIST | TETRA_RX_FLAG_AACH_SOFT)))
        return TETRA_ERR_ARG;
    // the AACH's soft decoding reads the soft ring, and a BBK row is decoded one way
    if ((cfg->flags & TETRA_RX_FLAG_AACH_SOFT) && (!(cfg->flags & TETRA_RX_FLAG_SOFT) || (cfg->flags & TETRA_RX_FLAG_AACH_RM3014))) return TETRA_ERR_ARG;
    std::unique_ptr<tetra_rx> h(new (std::nothrow) tetra_rx());      // everything it holds is released on every failure below
    if (!h) return TETRA_ERR_NOMEM;
    h->cfg = *cfg;
    h->cfg.demod.rrc_taps = h->cfg.demod.bandedge_taps = h->cfg.demod.interp_bank = nullptr;
    h->kinds = (cfg->kinds ? cfg->kinds : (1 << TETRA_RX_N_KINDS) - 1) | (1 << TETRA_RX_KIND_SB1);
    h->one_stream = (cfg->flags & TETRA_RX_FLAG_ONE_STREAM) != 0;
    h->aach_rm = (cfg->flags & TETRA_RX_FLAG_AACH_RM3014) != 0;
    h->soft = (cfg->flags & TETRA_RX_FLAG_SOFT) != 0;
    h->aach_soft = (cfg->flags & TETRA_RX_FLAG_AACH_SOFT) != 0;
    h->biterr = (cfg->flags & TETRA_RX_FLAG_BITERR) != 0;
    h->list = (cfg->flags & TETRA_RX_FLAG_LIST) != 0;
    h->list_T = TETRA_LIST_DEFAULT_CANDIDATES;
    TETRA_TRY(tetra_demod_create(&cfg->demod, h->dem.put()));
    h->C = cfg->demod.n_channels;
    int dev = cfg->demod.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return TETRA_ERR_NO_DEVICE;
    h->device = dev;
    DeviceGuard g(dev);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    h->stride = tetra_demod_bits_stride_for(h->dem, cfg->demod.max_samples);
    if (h->stride < 0) return h->stride;
    TETRA_TRY(tetra_bsync_create(h->C, h->stride, dev, h->bs.put()));
    h->F = tetra_bsync_max_frames(h->bs);
    if (cfg->flags & TETRA_RX_FLAG_SYNC_TOLERANT) {
        const tetra_bsync_tolerance_t tol = { TETRA_SYNC_TOL_DEFAULT_NORM, TETRA_SYNC_TOL_DEFAULT_SYNC, TETRA_SYNC_TOL_DEFAULT_MISS };
        TETRA_TRY(tetra_bsync_set_tolerance(h->bs, &tol));
    }
    const long long rows = (long long)h->C * h->F;
    if (rows > 0x7fffffffLL / 512) return TETRA_ERR_SIZE;      // 32-bit row / byte indices downstream
    h->rows = (int)rows;
    const size_t n = (size_t)rows;
    bool ok = hipStreamCreateWithFlags(h->tail.put(), hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(h->fetch_s.put(), hipStreamNonBlocking) == hipSuccess;
    for (int b = 0; b < 2 && ok; b++) {
        ok = dalloc(h->bits[b], (size_t)h->C * h->stride) && dalloc(h->nbits[b], (size_t)h->C) && dalloc(h->lists[b], (size_t)TETRA_N_LISTS * n) &&
             dalloc(h->counts[b], (size_t)TETRA_N_LISTS) && hipEventCreateWithFlags(h->ev_demod[b].put(), hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(h->ev_tail[b].put(), hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(h->ev_out[b].put(), hipEventDisableTiming) == hipSuccess;
        for (int k = 0; k < TETRA_RX_N_KINDS && ok; k++) {
            if (!(h->kinds & (1 << k))) continue;
            KindBufs& r = h->res[b][k];
            ok = dalloc(r.t2, n * kKinds[k].out_stride) && dalloc(r.ok, n) && dalloc(r.blocks, n) && row_col::alloc(h.get(), r, k, n ? n : 1);
            r.row_frame = h->lists[b] + (size_t)kKinds[k].list * n;
            r.n_rows = h->counts[b] + kKinds[k].list;
        }
    }
    ok = ok && dalloc(h->frames, n * TETRA_FRAME_WORDS) && dalloc(h->ft, n) && dalloc(h->fb, n) && dalloc(h->nf, (size_t)h->C) &&
         dalloc(h->chan_first, (size_t)TETRA_N_LISTS * h->C) && dalloc(h->index_work, (size_t)TETRA_N_LISTS * ((n + 255) / 256)) &&
         dalloc(h->row_scramb, n) && dalloc(h->row_time_rx, n) && dalloc(h->row_time, n) && dalloc(h->cell, (size_t)h->C);
    for (auto& e : h->ev_stage) ok = ok && hipEventCreate(e.put()) == hipSuccess;
    if (ok && chan_tab::status(h.get(), TAB_LINK) == TETRA_OK) ok = dalloc(h->link, (size_t)h->C);
    if (ok && h->soft) {
        h->soft_R = tetra_soft::ring_size(h->stride);
        ok = dalloc(h->sym, (size_t)h->C * h->stride) && dalloc(h->soft_ring, (size_t)h->C * h->soft_R) && dalloc(h->soft_prev, (size_t)4 * h->C) &&
             dalloc(h->soft_bits, (size_t)2 * h->C) && hipMemset(h->soft_ring, 0, (size_t)h->C * h->soft_R) == hipSuccess;
    }
    if (ok) {      // the decision scratch of the two decode launches (they run one after the other), sized for the worst case (every frame slot a row of every kind)
        tetra_lmac_job_t jobs[TETRA_RX_N_KINDS] = {};
        int nj = 0;
        for (int k : kJobOrder)
            if (h->kinds & (1 << k)) { jobs[nj].type = kKinds[k].tpsap; jobs[nj].blk_num = kKinds[k].blk; jobs[nj].max_rows = h->rows; nj++; }
        const size_t ws_bytes = tetra_lmac_decode_frames_workspace_bytes(jobs, nj);
        tetra_lmac_job_t sb1 = {};
        sb1.type = TETRA_TPSAP_T_SB1; sb1.blk_num = 1; sb1.max_rows = h->rows;
        const size_t sb1_bytes = tetra_lmac_decode_frames_workspace_bytes(&sb1, 1);
        ok = h->lmac_ws.reserve(sb1_bytes > ws_bytes ? sb1_bytes : ws_bytes) == hipSuccess;
        if (ok && h->list) {
            const size_t a = lmac_impl::list_work_bytes(jobs, nj), b1 = lmac_impl::list_work_bytes(&sb1, 1);
            ok = h->list_ws.reserve(a > b1 ? a : b1) == hipSuccess;
        }
    }
    if (!ok) return TETRA_ERR_NOMEM;
    TETRA_TRY(zero_results(h.get()));
    *out = h.release();
    return TETRA_OK;
}

int tetra_rx_destroy(tetra_rx_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return TETRA_OK;
}

int tetra_rx_reset(tetra_rx_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    TETRA_TRY(tetra_demod_reset(h->dem, -1));
    TETRA_TRY(tetra_bsync_reset(h->bs));
    TETRA_TRY(zero_results(h));
    h->calls = 0;
    h->soft_par = 0;
    h->stage_valid = false;
    for (bool& p : h->out_pending) p = false;          // (the device is idle: every delivery has completed)
    for (long long& c : h->ring_call) c = -1;
    h->snap_taken[0] = h->snap_taken[1] = 0;           // (the mask stays armed: the next tails take snapshots again)
    h->reset_pending = false;
    return TETRA_OK;
}

int tetra_rx_process_device(tetra_rx_t* h, const float* d_iq, int n_samples, void* hip_stream) {
    if (!h || (!d_iq && n_samples > 0)) return TETRA_ERR_ARG;
    if (n_samples < 0 || n_samples > h->cfg.demod.max_samples) return TETRA_ERR_SIZE;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t sa = static_cast<hipStream_t>(hip_stream);
    hipStream_t sb = h->one_stream ? sa : h->tail;
    const int b = (int)(h->calls & 1);
    // the bit rows of this parity were last read by the tail of call k - 2
    if (h->calls >= 2 && !h->one_stream) HIP_TRY(h, hipStreamWaitEvent(sa, h->ev_tail[b], 0));
    if (h->reset_pending) {         // channels reset since the last call (tetra_retune.h): the demodulator starts behind that
        HIP_TRY(h, hipStreamWaitEvent(sa, h->ev_reset, 0));
        h->reset_pending = false;
    }
    TETRA_TRY(tetra_demod_process_device(h->dem, d_iq, n_samples, h->bits[b], h->stride, h->nbits[b], h->soft ? h->sym.get() : nullptr, sa));
    if (h->soft) {      // behind the demodulator, in front of ev_demod: the tail finds the call's soft values in the ring
        const int p = h->soft_par, sym_stride = h->stride / 2;
        hipLaunchKernelGGL(k_soft, dim3((unsigned)((sym_stride + 255) / 256), (unsigned)h->C), dim3(256), 0, sa, reinterpret_cast<const float2*>(h->sym.get()),
                           sym_stride, h->nbits[b].get(), reinterpret_cast<const float2*>(h->soft_prev.get()) + (size_t)p * h->C, h->soft_bits + (size_t)p * h->C,
                           reinterpret_cast<float2*>(h->soft_prev.get()) + (size_t)(p ^ 1) * h->C, h->soft_bits + (size_t)(p ^ 1) * h->C, h->soft_ring.get(),
                           h->soft_R);
        HIP_TRY(h, hipGetLastError());
        h->soft_par = p ^ 1;
    }
    HIP_TRY(h, hipEventRecord(h->ev_demod[b], sa));
    if (!h->one_stream) HIP_TRY(h, hipStreamWaitEvent(sb, h->ev_demod[b], 0));
    h->calls++;                     // the call exists from here on: a failing tail leaves its rows undefined, not the bookkeeping
    h->stage_valid = false;
    // a delivery of call k - 2 (tetra_rx_out.h) still reads this parity's results: this tail waits for it on the device
    if (h->out_pending[b]) {
        HIP_TRY(h, hipStreamWaitEvent(sb, h->ev_out[b], 0));
        h->out_pending[b] = false;
    }
    // a table change since the last call (ext/tetra_traffic.h): this tail and every later one read the new table
    if (h->traffic && h->traffic->set_pending) {
        HIP_TRY(h, hipStreamWaitEvent(sb, h->traffic->ev_set, 0));
        h->traffic->set_pending = false;
    }
    TETRA_TRY(enqueue_tail(h, b, sb));
    HIP_TRY(h, hipEventRecord(h->ev_tail[b], sb));
    h->stage_valid = true;
    return TETRA_OK;
}

int tetra_rx_process(tetra_rx_t* h, const float* iq, int n_samples) {
    if (!h || (!iq && n_samples > 0)) return TETRA_ERR_ARG;
    if (n_samples < 0 || n_samples > h->cfg.demod.max_samples) return TETRA_ERR_SIZE;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    const size_t bytes = sizeof(float) * 2 * (size_t)h->C * (size_t)n_samples;
    if (h->st_iq.reserve(sizeof(float) * 2 * (size_t)h->C * (size_t)h->cfg.demod.max_samples) != hipSuccess) return TETRA_ERR_NOMEM;
    // the staging buffer is read by the demodulator launch of the previous call: wait for it before overwriting
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    if (bytes) HIP_TRY(h, hipMemcpy(h->st_iq, iq, bytes, hipMemcpyHostToDevice));
    return tetra_rx_process_device(h, h->st_iq, n_samples, nullptr);
}

int tetra_rx_wait(tetra_rx_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    for (int b = 0; b < 2; b++)
        if (h->calls > b) {
            HIP_TRY(h, hipEventSynchronize(h->ev_demod[b]));
            HIP_TRY(h, hipEventSynchronize(h->ev_tail[b]));
        }
    long long over = 0;
    TETRA_TRY(tetra_demod_get_overruns(h->dem, &over));
    return over > 0 ? TETRA_ERR_OVERRUN : TETRA_OK;
}

int tetra_rx_max_rows(tetra_rx_t* h) { return h ? h->rows : TETRA_ERR_ARG; }

int tetra_rx_fetch(tetra_rx_t* h, int which, int kind, tetra_rx_block_t* blocks, uint8_t* type1, int type1_stride, int capacity, int* n_rows) {
    if (!h || !n_rows || kind < 0 || kind >= TETRA_RX_N_KINDS || which < 0 || which > 1 || capacity < 0) return TETRA_ERR_ARG;
    if (!(h->kinds & (1 << kind))) return TETRA_ERR_UNSUPPORTED;
    if (type1 && type1_stride < kKinds[kind].type1_bits) return TETRA_ERR_SIZE;
    return fetch_rows(h, which, kind, blocks || type1, capacity, n_rows, [&](const KindBufs& r, int n) -> int {
        if (blocks) HIP_TRY(h, hipMemcpy(blocks, r.blocks, sizeof(tetra_rx_block_t) * (size_t)n, hipMemcpyDeviceToHost));
        if (type1) {
            const int nb = kKinds[kind].type1_bits;
            if (type1_stride == nb) {      // contiguous rows at the caller's
                const long long units = (long long)n * (nb >> 1);
                TETRA_TRY(fetch_packed(h, type1, (size_t)n * nb, [&](uint8_t* stage) {
                    hipLaunchKernelGGL(k_rx_pack_type1, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, h->fetch_s, r.t2.get(), kKinds[kind].out_stride, nb, n, stage);
                }));
            } else {
                HIP_TRY(h, hipMemcpy2D(type1, (size_t)type1_stride, r.t2, (size_t)kKinds[kind].out_stride, (size_t)nb, (size_t)n, hipMemcpyDeviceToHost));
            }
        }
        return TETRA_OK;
    });
}

int tetra_rx_fetch_aach_dist(tetra_rx_t* h, int which, uint8_t* dist, int capacity, int* n_rows) {
    return fetch_col(h, which, TETRA_RX_KIND_BBK, COL_AACH_DIST, dist, capacity, n_rows);
}

// the chain's share of ext/tetra_aach_soft.h
int tetra_rx_set_aach_min_margin(tetra_rx_t* h, int min_margin) {
    if (!h) return TETRA_ERR_ARG;
    if (!h->aach_soft) return TETRA_ERR_UNSUPPORTED;
    if (min_margin < 1 || min_margin > TETRA_AACH_SOFT_MAX_MARGIN) return TETRA_ERR_ARG;
    h->aach_min_margin = min_margin;
    return TETRA_OK;
}

// byte 31 of the BBK rows, packed on the device as the distance is and widened on the host
int tetra_rx_fetch_aach_margin(tetra_rx_t* h, int which, uint16_t* margin, int capacity, int* n_rows) {
    if (!h || !n_rows || which < 0 || which > 1 || capacity < 0) return TETRA_ERR_ARG;
    if (!h->aach_soft) return TETRA_ERR_UNSUPPORTED;
    TETRA_TRY(row_col::status(h, COL_AACH_DIST, TETRA_RX_KIND_BBK));
    return fetch_rows(h, which, TETRA_RX_KIND_BBK, margin != nullptr, capacity, n_rows, [&](const KindBufs& r, int n) -> int {
        std::vector<uint8_t> bytes((size_t)n);
        TETRA_TRY(fetch_packed(h, bytes.data(), (size_t)n, [&](uint8_t* stage) {
            hipLaunchKernelGGL(k_rx_pack_byte, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->fetch_s, r.t2.get(), kKinds[TETRA_RX_KIND_BBK].out_stride,
                               kAachMarginByte, n, stage);
        }));
        for (int j = 0; j < n; ++j) margin[j] = bytes[(size_t)j];
        return TETRA_OK;
    });
}

// the chain's share of tetra_biterr.h
int tetra_rx_fetch_biterr(tetra_rx_t* h, int which, int kind, uint32_t* out, int capacity, int* n_rows) {
    return fetch_col(h, which, kind, COL_BITERR, out, capacity, n_rows);
}

int tetra_rx_biterr_device(tetra_rx_t* h, int which, int kind, const uint32_t** d_biterr, void* hip_stream) {
    return col_device(h, which, kind, COL_BITERR, d_biterr, hip_stream);
}

int tetra_rx_get_link(tetra_rx_t* h, int first, int count, tetra_rx_link_t* out) { return get_chan(h, TAB_LINK, first, count, out); }

// the chain's share of tetra_list.h
int tetra_rx_set_list_candidates(tetra_rx_t* h, int max_candidates) {
    if (!h) return TETRA_ERR_ARG;
    if (!h->list) return TETRA_ERR_UNSUPPORTED;
    if (max_candidates < 1 || max_candidates > TETRA_LIST_MAX_CANDIDATES) return TETRA_ERR_ARG;
    h->list_T = max_candidates;
    return TETRA_OK;
}

int tetra_rx_fetch_list_rank(tetra_rx_t* h, int which, int kind, int32_t* out, int capacity, int* n_rows) {
    return fetch_col(h, which, kind, COL_RANK, out, capacity, n_rows);
}

int tetra_rx_list_rank_device(tetra_rx_t* h, int which, int kind, const int32_t** d_rank, void* hip_stream) {
    return col_device(h, which, kind, COL_RANK, d_rank, hip_stream);
}

int tetra_rx_rows_device(tetra_rx_t* h, int which, int kind, const uint8_t** d_type2, int* type2_stride, const tetra_rx_block_t** d_blocks,
                         const int32_t** d_n_rows, void* hip_stream) {
    if (!h || kind < 0 || kind >= TETRA_RX_N_KINDS || which < 0 || which > 1) return TETRA_ERR_ARG;
    if (!(h->kinds & (1 << kind))) return TETRA_ERR_UNSUPPORTED;
    const int b = parity_of(h, which);
    if (b < 0) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), h->ev_tail[b], 0));
    const KindBufs& r = h->res[b][kind];
    if (d_type2) *d_type2 = r.t2;
    if (type2_stride) *type2_stride = kKinds[kind].out_stride;
    if (d_blocks) *d_blocks = r.blocks;
    if (d_n_rows) *d_n_rows = r.n_rows;
    return TETRA_OK;
}

int tetra_rx_get_cell(tetra_rx_t* h, int first, int count, tetra_lmac_cell_state_t* out) { return get_chan(h, TAB_CELL, first, count, out); }

int tetra_rx_get_sync_state(tetra_rx_t* h, int first, int count, tetra_bsync_state_t* out) { return get_chan(h, TAB_SYNC_STATE, first, count, out); }

// the chain's share of tetra_handover.h: the first three words of every channel's hand-over fields; all zero on a handle without them
int tetra_rx_get_handover(tetra_rx_t* h, int first, int count, tetra_handover_status_t* out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    if (!h || !out || first < 0 || count < 0 || first + (long long)count > h->C) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    TETRA_TRY(latest_tail_done(h));
    if (h->calls == 0) HIP_TRY(h, hipDeviceSynchronize());      // (no tail yet whose event a hand-over would have been recorded behind)
    void* live = nullptr;
    TETRA_TRY(chan_tab::live(h, TAB_HANDOVER, &live));
    std::vector<bsync_core::Assist> fields((size_t)count, bsync_core::Assist{});
    if (live && count)
        HIP_TRY(h, hipMemcpy(fields.data(), static_cast<const bsync_core::Assist*>(live) + first, sizeof(bsync_core::Assist) * (size_t)count, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; i++) out[i] = { fields[(size_t)i].status, fields[(size_t)i].waited, fields[(size_t)i].offset };
    return TETRA_OK;
}

// the chain's share of tetra_sync_tol.h
int tetra_rx_set_sync_tolerance(tetra_rx_t* h, const tetra_bsync_tolerance_t* tol) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    TETRA_TRY(latest_tail_done(h));      // (the synchroniser's own entry waits for the device)
    return tetra_bsync_set_tolerance(h->bs, tol);
}

int tetra_rx_get_sync_misses(tetra_rx_t* h, int first, int count, int32_t* out) { return get_chan(h, TAB_SYNC_MISSES, first, count, out); }

int tetra_rx_bits_device(tetra_rx_t* h, int which, const uint8_t** d_bits, int* bits_stride, const int32_t** d_n_bits, void* hip_stream) {
    if (!h || which < 0 || which > 1) return TETRA_ERR_ARG;
    const int b = parity_of(h, which);
    if (b < 0) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), h->ev_demod[b], 0));
    if (d_bits) *d_bits = h->bits[b];
    if (bits_stride) *bits_stride = h->stride;
    if (d_n_bits) *d_n_bits = h->nbits[b];
    return TETRA_OK;
}

tetra_demod_t* tetra_rx_demod(tetra_rx_t* h) { return h ? h->dem : nullptr; }

int tetra_rx_stage_ms(tetra_rx_t* h, float ms[4]) {
    if (!h || !ms || !h->stage_valid) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipEventSynchronize(h->ev_stage[3]));
    TETRA_TRY(tetra_demod_last_kernel_ms(h->dem, &ms[0]));
    for (int i = 0; i < 3; i++) HIP_TRY(h, hipEventElapsedTime(&ms[1 + i], h->ev_stage[i], h->ev_stage[i + 1]));
    return TETRA_OK;
}

}  // extern "C"
