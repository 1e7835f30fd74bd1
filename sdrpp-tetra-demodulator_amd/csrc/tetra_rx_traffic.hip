// tetra_rx_traffic.hip -- the receive chain decodes the traffic slots the host names as TCH blocks (include/ext/tetra_traffic.h).
//
// Behind the tail's last decode launch and its link figures, per call: the rule of traffic_core.hpp over the entries of the call's
// TETRA_LIST_ANY -- entry j is BBK row j and names its frame -- as a three-list compaction (compact_core.hpp: count / scan / write;
// the lists come out in (channel, frame) order without atomics), each list clamped at the handle's max_rows on the device, then ONE
// more lmac_impl::decode_frames call with up to three TCH jobs over those lists (two calls with TETRA_RX_FLAG_SOFT: TCH/7.2 is
// not coded and stays a hard job from the packed frames).  Every kernel here is a 256-thread workgroup of at most 26 vector registers
// and 256 bytes of LDS, so that it fits beside the demodulator on a compute unit.
// A source of its own: every other source's device code is what it was.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <new>

#include "../../include/ext/tetra_traffic.h"
#include "compact_core.hpp"
#include "lmac_impl.hpp"
#include "rx_handle.hpp"
#include "traffic_core.hpp"

namespace {

using traffic_core::Slot;
static_assert(sizeof(Slot) == sizeof(tetra_rx_traffic_slot_t) && sizeof(Slot) == sizeof(int32_t), "a table entry is one word of the staging ring");
static_assert(traffic_core::kKinds == kTrafficKinds && traffic_core::kFirstKind == TETRA_LMAC_T_TCH_7_2 && TETRA_LMAC_T_TCH_2_4 == TETRA_LMAC_T_TCH_7_2 + 2,
              "list k holds TETRA_LMAC_T_TCH_7_2 + k");
static_assert(traffic_core::kTrainNorm1 == TETRA_TRAIN_NORM_1, "rule (a)");

constexpr int kRows = 256;                     // entries per workgroup of the count and write kernels
constexpr int kStride[kTrafficKinds] = { 432, 296, 152 }, kType2[kTrafficKinds] = { 432, 292, 148 };
constexpr int kBbkStride = kKinds[TETRA_RX_KIND_BBK].out_stride;

// what the rule reads of a call: entry j < *n_any of the ANY list is frame any_list[j] and BBK row j (bbk_*: null on a handle without BBK rows)
struct RouteArgs {
    const int32_t* any_list;
    const int32_t* n_any;
    const int32_t* frame_type;
    const uint32_t* row_scramb;
    const uint32_t* row_time;
    const Slot* table;            // [rows / F][4]
    const uint8_t* bbk_t2;
    const int32_t* bbk_ok;
    int F, rows;
};
// entry j -> its frame and the K-bit mask of compact_core (at most one bit: the list its TCH row goes to)
__device__ __forceinline__ unsigned route_entry(const RouteArgs& a, int j, int& frame) {
    frame = -1;
    if (j >= min(*a.n_any, a.rows)) return 0u;
    const int r = a.any_list[j];
    if (r < 0 || r >= a.rows) return 0u;
    frame = r;
    const int k = traffic_core::route(a.frame_type[r], a.row_scramb[r], a.row_time[r], a.table + (size_t)(r / a.F) * 4, a.bbk_ok ? a.bbk_ok[j] : 0,
                                      a.bbk_t2 ? a.bbk_t2 + (size_t)j * kBbkStride : nullptr);
    return k < 0 ? 0u : 1u << k;
}

// 1. routed entries per kRows entries and list
__global__ __launch_bounds__(kRows) void k_traffic_count(const RouteArgs a, int nblocks, int* __restrict__ work) {
    int frame;
    const unsigned m = route_entry(a, (int)blockIdx.x * kRows + (int)threadIdx.x, frame);
    compact_core::block_count<kTrafficKinds>(m, work, nblocks, blockIdx.x);
}
// 2. exclusive scan of each list's block counts; the totals, clamped -> counts [kind][routed, kept, dropped]
__global__ __launch_bounds__(compact_core::kScanThreads) void k_traffic_scan(int* __restrict__ work, int nblocks, int max_rows, int32_t* __restrict__ counts) {
    __shared__ int totals[kTrafficKinds];
    int len[kTrafficKinds];
#pragma unroll
    for (int k = 0; k < kTrafficKinds; ++k) len[k] = nblocks;
    compact_core::scan_counts<kTrafficKinds>(work, nblocks, len, totals);
    if (threadIdx.x == compact_core::kScanThreads - 1)          // (the thread that wrote the totals)
        for (int k = 0; k < kTrafficKinds; ++k) traffic_core::clamp_counts(totals[k], max_rows, counts + traffic_core::kCounts * k);
}
// 3. the lists [kind][max_rows]: the first max_rows routed frames of each
__global__ __launch_bounds__(kRows) void k_traffic_write(const RouteArgs a, int nblocks, int max_rows, const int* __restrict__ work, int32_t* __restrict__ lists) {
    int frame;
    const unsigned m = route_entry(a, (int)blockIdx.x * kRows + (int)threadIdx.x, frame);
    int at[kTrafficKinds];
    compact_core::block_rank<kTrafficKinds, kRows>(m, at);
#pragma unroll
    for (int k = 0; k < kTrafficKinds; ++k) {
        const int pos = at[k] + work[k * nblocks + blockIdx.x];
        if (((m >> k) & 1u) && traffic_core::kept(pos, max_rows)) lists[(size_t)k * max_rows + pos] = frame;
    }
}

int list_of(int tch_kind) { return tch_kind >= TETRA_LMAC_T_TCH_7_2 && tch_kind <= TETRA_LMAC_T_TCH_2_4 ? tch_kind - TETRA_LMAC_T_TCH_7_2 : -1; }
bool coded(int k) { return k != 0; }

// what every entry point but enable checks first
int usable(const tetra_rx* h) { return !h ? TETRA_ERR_ARG : !h->traffic ? TETRA_ERR_UNSUPPORTED : TETRA_OK; }

int parity(const tetra_rx* h, int which) { return h->calls <= which ? -1 : (int)((h->calls - 1 - which) & 1); }

}  // namespace

int traffic_impl::enqueue(tetra_rx* h, int b, hipStream_t s) {
    TrafficState& t = *h->traffic;
    const bool bbk = (h->kinds & (1 << TETRA_RX_KIND_BBK)) != 0;
    const KindBufs& rb = h->res[b][TETRA_RX_KIND_BBK];
    const RouteArgs a = { h->lists[b] + (size_t)TETRA_LIST_ANY * (size_t)h->rows, h->counts[b] + TETRA_LIST_ANY, h->ft, h->row_scramb, h->row_time,
                          reinterpret_cast<const Slot*>(t.table.get()), bbk ? rb.t2.get() : nullptr, bbk ? rb.ok.get() : nullptr, h->F, h->rows };
    const int nblocks = (h->rows + kRows - 1) / kRows;
    if (nblocks == 0) return TETRA_OK;
    hipLaunchKernelGGL(k_traffic_count, dim3((unsigned)nblocks), dim3(kRows), 0, s, a, nblocks, t.work.get());
    hipLaunchKernelGGL(k_traffic_scan, dim3(1), dim3(compact_core::kScanThreads), 0, s, t.work.get(), nblocks, t.max_rows, t.counts[b].get());
    hipLaunchKernelGGL(k_traffic_write, dim3((unsigned)nblocks), dim3(kRows), 0, s, a, nblocks, t.max_rows, t.work.get(), t.lists[b].get());
    HIP_TRY(h, hipGetLastError());
    tetra_lmac_frames_t src = {};
    src.d_frames = h->frames;
    src.d_frame_type = h->ft;
    src.n_frames = h->rows;
    src.frames_per_channel = h->F;
    src.d_frame_bitnum = h->fb;
    src.d_time_rx = h->row_time_rx;
    src.d_time = h->row_time;
    src.d_workspace = t.ws;
    src.workspace_bytes = t.ws.bytes();
    tetra_lmac_job_t jobs[kTrafficKinds];
    uint32_t* counts[kTrafficKinds];
    auto job_of = [&](int k) {
        const TrafficBufs& r = t.res[b][k];
        tetra_lmac_job_t j = {};
        j.type = TETRA_LMAC_T_TCH_7_2 + k;
        j.d_row_frame = t.lists[b] + (size_t)k * (size_t)t.max_rows;
        j.d_n_rows = t.counts[b] + traffic_core::kCounts * k + 1;      // the rows kept
        j.max_rows = t.max_rows;
        j.out_stride = kStride[k];
        j.d_frame_scramb = h->row_scramb;
        j.d_type2 = r.t2;
        j.d_crc_ok = r.ok;
        j.d_labels = reinterpret_cast<tetra_lmac_label_t*>(r.blocks.get());
        return j;
    };
    const lmac_impl::SoftRing ring = { h->soft_ring, h->soft_R };
    lmac_impl::FrameOpts hard, soft;
    hard.d_biterr = soft.d_biterr = h->biterr ? counts : nullptr;
    soft.soft = &ring;
    soft.soft_tch = true;
    int nj = 0;
    // long blocks first; with soft values TCH/7.2, which is not coded, in a call of its own from the packed frames
    for (int k : { 1, 2, 0 }) {
        if (h->soft && k == 0) {
            TETRA_TRY(lmac_impl::decode_frames(&src, jobs, nj, soft, s));
            nj = 0;
        }
        counts[nj] = coded(k) ? t.res[b][k].biterr.get() : nullptr;
        jobs[nj++] = job_of(k);
    }
    return lmac_impl::decode_frames(&src, jobs, nj, hard, s);
}

extern "C" {

int tetra_rx_traffic_enable(tetra_rx_t* h, int max_rows) {
    if (!h || h->traffic || max_rows < 1 || max_rows > h->rows) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    std::unique_ptr<TrafficState> t(new (std::nothrow) TrafficState());
    if (!t) return TETRA_ERR_NOMEM;
    t->max_rows = max_rows;
    const size_t n = (size_t)max_rows, nblocks = ((size_t)h->rows + kRows - 1) / kRows;
    bool ok = true;
    for (int b = 0; b < 2 && ok; b++) {
        ok = t->lists[b].reserve(sizeof(int32_t) * kTrafficKinds * n) == hipSuccess &&
             t->counts[b].reserve(sizeof(int32_t) * kTrafficKinds * traffic_core::kCounts) == hipSuccess &&
             hipMemset(t->counts[b], 0, sizeof(int32_t) * kTrafficKinds * traffic_core::kCounts) == hipSuccess;
        for (int k = 0; k < kTrafficKinds && ok; k++) {
            TrafficBufs& r = t->res[b][k];
            ok = r.t2.reserve(n * kStride[k]) == hipSuccess && r.ok.reserve(sizeof(int32_t) * n) == hipSuccess &&
                 r.blocks.reserve(sizeof(tetra_rx_block_t) * n) == hipSuccess &&
                 (!h->biterr || !coded(k) || r.biterr.reserve(sizeof(uint32_t) * n) == hipSuccess);
        }
    }
    tetra_lmac_job_t jobs[kTrafficKinds] = {};
    for (int k = 0; k < kTrafficKinds; k++) { jobs[k].type = TETRA_LMAC_T_TCH_7_2 + k; jobs[k].max_rows = max_rows; }
    const size_t ws = tetra_lmac_decode_frames_workspace_bytes(jobs, kTrafficKinds);
    ok = ok && t->work.reserve(sizeof(int32_t) * kTrafficKinds * (nblocks ? nblocks : 1)) == hipSuccess &&
         t->table.reserve(sizeof(Slot) * 4 * (size_t)h->C) == hipSuccess && hipMemset(t->table, 0, sizeof(Slot) * 4 * (size_t)h->C) == hipSuccess &&
         t->ws.reserve(ws ? ws : 4) == hipSuccess && hipEventCreateWithFlags(t->ev_set.put(), hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        return TETRA_ERR_NOMEM;
    }
    HIP_TRY(h, hipDeviceSynchronize());
    h->traffic = std::move(t);
    return TETRA_OK;
}

int tetra_rx_set_traffic(tetra_rx_t* h, int first, int count, const tetra_rx_traffic_slot_t* slots, void* hip_stream) {
    TETRA_TRY(usable(h));
    if (first < 0 || count < 0 || first + (long long)count > h->C || (count && !slots)) return TETRA_ERR_ARG;
    const bool bbk = (h->kinds & (1 << TETRA_RX_KIND_BBK)) != 0;
    for (int i = 0; i < count * 4; i++) {
        const Slot s = { slots[i].kind, slots[i].usage, { 0, 0 } };
        if (!traffic_core::slot_valid(s) || (s.usage && !bbk)) return TETRA_ERR_ARG;
    }
    if (!count) return TETRA_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    TrafficState& t = *h->traffic;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // behind the tail of every call enqueued so far (tails run one after the other), and behind an earlier change still on its way
    if (h->calls > 0) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_tail[(h->calls - 1) & 1], 0));
    if (t.set_pending) HIP_TRY(h, hipStreamWaitEvent(s, t.ev_set, 0));
    int32_t words[64];
    std::unique_ptr<int32_t[]> big;
    int32_t* w = words;
    if (count * 4 > 64) {
        big.reset(new (std::nothrow) int32_t[(size_t)count * 4]);
        if (!big) return TETRA_ERR_NOMEM;
        w = big.get();
    }
    for (int i = 0; i < count * 4; i++) {
        const Slot e = { slots[i].kind, slots[i].usage, { 0, 0 } };
        std::memcpy(&w[i], &e, sizeof(e));
    }
    int32_t* d_list = nullptr;
    hipError_t err = hipSuccess;
    const int k = t.to_device.push(w, count * 4, h->C * 4, s, &d_list, &err);
    if (k < 0) HIP_TRY(h, err);
    HIP_TRY(h, hipMemcpyAsync(t.table.get() + sizeof(Slot) * 4 * (size_t)first, d_list, sizeof(Slot) * 4 * (size_t)count, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, t.to_device.done(k, 0, s));
    HIP_TRY(h, hipEventRecord(t.ev_set, s));
    t.set_pending = t.ever_set = true;
    return TETRA_OK;
}

int tetra_rx_get_traffic(tetra_rx_t* h, int first, int count, tetra_rx_traffic_slot_t* slots) {
    TETRA_TRY(usable(h));
    if (first < 0 || count < 0 || first + (long long)count > h->C || (count && !slots)) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    TrafficState& t = *h->traffic;
    if (t.ever_set) HIP_TRY(h, hipEventSynchronize(t.ev_set));
    if (count) HIP_TRY(h, hipMemcpy(slots, t.table.get() + sizeof(Slot) * 4 * (size_t)first, sizeof(Slot) * 4 * (size_t)count, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

int tetra_rx_fetch_traffic(tetra_rx_t* h, int which, int tch_kind, tetra_rx_block_t* blocks, uint8_t* type2, int stride, int capacity, uint32_t* biterr,
                           int* n_rows, int* n_dropped) {
    TETRA_TRY(usable(h));
    const int k = list_of(tch_kind);
    if (!n_rows || k < 0 || which < 0 || which > 1 || capacity < 0) return TETRA_ERR_ARG;
    if (biterr && (!h->biterr || !coded(k))) return TETRA_ERR_UNSUPPORTED;
    if (type2 && stride < kType2[k]) return TETRA_ERR_SIZE;
    *n_rows = 0;
    if (n_dropped) *n_dropped = 0;
    const int b = parity(h, which);
    if (b < 0) return TETRA_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipEventSynchronize(h->ev_tail[b]));
    const TrafficState& t = *h->traffic;
    int32_t c[traffic_core::kCounts] = {};
    HIP_TRY(h, hipMemcpy(c, t.counts[b] + traffic_core::kCounts * k, sizeof(c), hipMemcpyDeviceToHost));
    if (c[1] < 0 || c[1] > t.max_rows || c[2] < 0) return TETRA_ERR_HIP;      // (cannot happen: the clamp is on the device)
    *n_rows = c[1];
    if (n_dropped) *n_dropped = c[2];
    const bool wants = blocks || type2 || biterr;
    if (c[1] > capacity) return wants ? TETRA_ERR_SIZE : TETRA_OK;
    if (!c[1] || !wants) return TETRA_OK;
    const TrafficBufs& r = t.res[b][k];
    const size_t n = (size_t)c[1];
    if (blocks) HIP_TRY(h, hipMemcpy(blocks, r.blocks, sizeof(tetra_rx_block_t) * n, hipMemcpyDeviceToHost));
    if (type2) HIP_TRY(h, hipMemcpy2D(type2, (size_t)stride, r.t2, (size_t)kStride[k], (size_t)kType2[k], n, hipMemcpyDeviceToHost));
    if (biterr) HIP_TRY(h, hipMemcpy(biterr, r.biterr, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

int tetra_rx_traffic_rows_device(tetra_rx_t* h, int which, int tch_kind, const uint8_t** d_type2, int* type2_stride, const tetra_rx_block_t** d_blocks,
                                 const int32_t** d_counts, const uint32_t** d_biterr, void* hip_stream) {
    TETRA_TRY(usable(h));
    const int k = list_of(tch_kind);
    if (k < 0 || which < 0 || which > 1) return TETRA_ERR_ARG;
    const int b = parity(h, which);
    if (b < 0) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), h->ev_tail[b], 0));
    const TrafficState& t = *h->traffic;
    const TrafficBufs& r = t.res[b][k];
    if (d_type2) *d_type2 = r.t2;
    if (type2_stride) *type2_stride = kStride[k];
    if (d_blocks) *d_blocks = r.blocks;
    if (d_counts) *d_counts = t.counts[b] + traffic_core::kCounts * k;
    if (d_biterr) *d_biterr = r.biterr;
    return TETRA_OK;
}

}  // extern "C"
