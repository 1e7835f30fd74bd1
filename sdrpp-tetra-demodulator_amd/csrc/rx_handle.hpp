// rx_handle.hpp -- the receive-chain handle (include/tetra_rx.h) as its C ABI sources share it: tetra_rx.hip runs the chain,
// tetra_rx_out.hip delivers a call's results to the host (include/tetra_rx_out.h).  Host-side definitions only.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>

#include "../../include/ext/tetra_biterr.h"
#include "../../include/tetra_rx.h"
#include "bsync_core.hpp"
#include "hip_host.hpp"
#include "retune_impl.hpp"
#include "retune_list.hpp"
#include "rx_out_core.hpp"

namespace tetra_rx_impl {

struct KindInfo {
    int tpsap, blk, list, out_stride, type1_bits;
};
// rows as the decoder writes them (tetra_lower_mac.c:58-105: type2 / type1 bits) and the frame list a kind's rows come from
constexpr KindInfo kKinds[TETRA_RX_N_KINDS] = {
    { TETRA_TPSAP_T_SB1, 1, TETRA_LIST_SYNC, 80, 60 },       // SB1
    { TETRA_TPSAP_T_BBK, 0, TETRA_LIST_ANY, 32, 30 },        // BBK
    { TETRA_TPSAP_T_SB2, 2, TETRA_LIST_SYNC, 144, 124 },     // SB2
    { TETRA_TPSAP_T_NDB, 1, TETRA_LIST_NORM_2, 144, 124 },   // NDB blk 1
    { TETRA_TPSAP_T_NDB, 2, TETRA_LIST_NORM_2, 144, 124 },   // NDB blk 2
    { TETRA_TPSAP_T_SCH_F, 0, TETRA_LIST_NORM_1, 288, 268 }, // SCH/F
};
// the second decode launch's job order: long blocks first, so that the short ones fill the machine while the long ones finish
constexpr int kJobOrder[] = { TETRA_RX_KIND_SCH_F, TETRA_RX_KIND_SB2, TETRA_RX_KIND_NDB1, TETRA_RX_KIND_NDB2, TETRA_RX_KIND_BBK };

static_assert(sizeof(tetra_rx_block_t) == sizeof(tetra_lmac_label_t), "tetra_rx_block_t is the decoder's row label");

struct KindBufs {                 // one parity's results of one kind
    DevMem<uint8_t> t2;           // [rows][out_stride]
    DevMem<int32_t> ok;           // [rows]
    DevMem<tetra_rx_block_t> blocks;      // [rows]
    DevMem<uint32_t> biterr;              // [rows] errors | compared << 16 (TETRA_RX_FLAG_BITERR, coded kinds only)
    DevMem<int32_t> rank;                 // [rows] 0 / rank / -1 (TETRA_RX_FLAG_LIST, coded kinds only)
    // into the parity's frame lists (not owned): the kind's rows are the frames row_frame[0 .. *n_rows)
    const int32_t* row_frame = nullptr;
    const int32_t* n_rows = nullptr;
};

// The opt-in row columns and the per-channel tables in rx_out's order (rx_out::kRowCols, kChanTables; row_extra / chan_extra are their
// delivery bits, row_elem_bytes / chan_elem_bytes their element sizes, kind_has which kinds carry a column).  What this handle has
// of them and where it lies is stated once, in row_col and chan_tab behind the handle below.
enum { COL_BITERR, COL_RANK, COL_AACH_DIST };
enum { TAB_CELL, TAB_SYNC_STATE, TAB_SYNC_MISSES, TAB_LINK };
// ... and one more per-channel table behind rx_out's four, which no delivery or snapshot carries: the hand-over's fields
// (bsync_core::Assist, ext/tetra_handover.h), the synchroniser's like the two above
constexpr int TAB_HANDOVER = rx_out::kChanTables, kChanTablesAll = rx_out::kChanTables + 1;
// the Reed-Muller distance of a BBK row (TETRA_RX_FLAG_AACH_RM3014): the byte behind its 30 type-1 bits (tetra_aach.h)
// (TETRA_RX_FLAG_AACH_SOFT: the disagreeing soft values there, and the margin in the byte behind it, ext/tetra_aach_soft.h)
constexpr int kAachDistByte = 30, kAachMarginByte = 31;
struct ColSrc {                   // a column of one kind and parity on the device: element j at base + j * stride
    const uint8_t* base;
    size_t stride;
};

// ext/tetra_traffic.h (tetra_rx_traffic.hip): what tetra_rx_traffic_enable allocates.  List k holds TETRA_LMAC_T_TCH_7_2 + k.
constexpr int kTrafficKinds = 3;
struct TrafficBufs {              // one parity's rows of one TCH kind
    DevMem<uint8_t> t2;           // [max_rows][stride]
    DevMem<int32_t> ok;           // [max_rows] (all 1: the decoder's verdict for a block without a CRC)
    DevMem<tetra_rx_block_t> blocks;      // [max_rows]
    DevMem<uint32_t> biterr;              // [max_rows] (TETRA_RX_FLAG_BITERR, the two coded kinds)
};
struct TrafficState {
    int max_rows = 0;
    TrafficBufs res[2][kTrafficKinds];
    DevMem<int32_t> lists[2];             // [kTrafficKinds][max_rows] routed frames
    DevMem<int32_t> counts[2];            // [kTrafficKinds][3] routed, kept, dropped
    DevMem<int32_t> work;                 // [kTrafficKinds][blocks of 256 entries] the compaction's words
    DevMem<uint8_t> table;                // [C][4] tetra_rx_traffic_slot_t
    DevMem<void> ws;                      // the TCH decode launch's decision scratch
    ListRing to_device;                   // table entries on their way to the device
    Event ev_set;                         // the latest tetra_rx_set_traffic's copy into the table ...
    bool set_pending = false;             // ... which the next tail waits for on its stream
    bool ever_set = false;
};

}  // namespace tetra_rx_impl

using namespace tetra_rx_impl;

struct tetra_rx {
    tetra_rx_config_t cfg;
    int device = 0, last_hip = 0;
    int C = 0, F = 0, rows = 0, stride = 0, kinds = 0;
    bool one_stream = false;
    bool aach_rm = false;                 // TETRA_RX_FLAG_AACH_RM3014: the BBK job decodes with the AACH's Reed-Muller code (tetra_aach.h)
    // TETRA_RX_FLAG_SOFT (soft_core.hpp): the coded kinds decode from soft values.  All of it lives on the demodulator's stream.
    bool soft = false;
    bool aach_soft = false;               // TETRA_RX_FLAG_AACH_SOFT: the BBK job under `soft` is the maximum-likelihood one (ext/tetra_aach_soft.h)
    int aach_min_margin = 1;              // tetra_rx_set_aach_min_margin
    uint32_t soft_R = 0;                  // bits per channel's ring
    int soft_par = 0;                     // which half of soft_prev / soft_bits the next call reads (it writes the other)
    DevMem<float> sym;                    // [C][stride / 2] complex64: the call's symbols (one buffer: k_soft reads it behind the demodulator)
    DevMem<int8_t> soft_ring;             // [C][soft_R]
    DevMem<float> soft_prev;              // [2][C] complex64: a channel's last symbol
    DevMem<uint32_t> soft_bits;           // [2][C]: its absolute bit count = the synchroniser's numbering
    // TETRA_RX_FLAG_BITERR (tetra_biterr.h): the decode launches count channel bit errors per row, a kernel behind them sums them per channel
    bool biterr = false;
    DevMem<tetra_rx_link_t> link;         // [C], accumulated by the tails (one at a time, on one stream), zeroed by the resets
    // TETRA_RX_FLAG_LIST (tetra_list.h): the decode launches are followed by the rescue of their CRC-failed rows
    bool list = false;
    int list_T = 4;                       // tetra_rx_set_list_candidates
    DevMem<void> list_ws;                 // the list launches' compaction words (lmac_impl::list_work_bytes of the larger decode launch)
    Handle<tetra_demod_t*, tetra_demod_destroy> dem;
    Handle<tetra_bsync_t*, tetra_bsync_destroy> bs;
    Stream tail;
    Stream fetch_s;                       // tetra_rx_fetch's pack + copy (never behind a queued tail)
    // per call parity
    DevMem<uint8_t> bits[2];
    DevMem<int32_t> nbits[2];
    KindBufs res[2][TETRA_RX_N_KINDS];
    DevMem<int32_t> lists[2];             // [TETRA_N_LISTS][rows] frame lists
    DevMem<int32_t> counts[2];            // [TETRA_N_LISTS]
    Event ev_demod[2], ev_tail[2];
    // the tail's working set (one: tails run one after the other on one stream)
    DevMem<uint32_t> frames;              // [rows][16] packed frames
    DevMem<int32_t> ft;                   // [rows] frame types
    DevMem<uint32_t> fb;                  // [rows] frame bit numbers
    DevMem<int32_t> nf;                   // [C]
    DevMem<int32_t> chan_first;           // [TETRA_N_LISTS][C] position in each list of a channel's first entry
    DevMem<int32_t> index_work;           // tetra_burst_index_device's scratch
    DevMem<void> lmac_ws;                 // the decoder's decision scratch for the launch of every other kind
    DevMem<uint8_t> fetch_stage;          // tetra_rx_fetch: a kind's type-1 bits packed row after row (allocated on first use)
    DevMem<uint32_t> row_scramb, row_time_rx, row_time;
    DevMem<tetra_lmac_cell_state_t> cell; // [C]
    DevMem<float> st_iq;                  // host-path staging
    Event ev_stage[4];
    long long calls = 0;
    bool stage_valid = false;
    // deliveries (tetra_rx_out.hip), on fetch_s behind the tail of the call they read
    Event ev_out[2];                      // per call parity: the latest delivery of that parity's results ...
    bool out_pending[2] = { false, false };   // ... still to be waited for by the tail that overwrites those results
    static constexpr int kOutRing = 8;    // the latest deliveries, for tetra_rx_out_query / _wait (created on first use)
    Event ring_ev[kOutRing];
    long long ring_call[kOutRing] = { -1, -1, -1, -1, -1, -1, -1, -1 }, ring_seq[kOutRing] = {}, out_seq = 0;
    DevMem<int32_t> out_tiles;            // [TETRA_RX_N_KINDS][tiles]: kept rows per tile, scanned in place to their first output row
    DevMem<uint8_t> out_layout;           // the layout the write launch reads (rx_out::Layout)
    // the extension block (include/ext/tetra_rx_out_ext.h)
    DevMem<uint8_t> out_ext_layout;       // what the extras' layout launch leaves for their write launch
    int snap_mask = 0;                    // tetra_rx_out_set_snapshot: the channel extras every tail copies ...
    DevMem<uint8_t> snap[2];              // ... into its parity's snapshot (rx_out::snap_offset; allocated when first armed)
    int snap_taken[2] = { 0, 0 };         // the mask the latest tail of each parity ran with (0 again after a reset)
    // resets of single channels (include/tetra_retune.h, tetra_retune.hip)
    ListRing to_device;                       // the channel lists on their way to the device
    Event ev_reset;                       // the latest reset's work on the stream it was given ...
    bool reset_pending = false;           // ... which the next process call waits for on ITS stream
    bool owned = false;                   // inside a wideband handle (tetra_wbrx_rx): that handle restarts its channels, the entry point refuses
    std::unique_ptr<TrafficState> traffic;    // ext/tetra_traffic.h: null until tetra_rx_traffic_enable
};

// tetra_rx_traffic.hip: the routing and the TCH decode of call parity b behind the tail's other launches on s (a handle with `traffic`)
namespace traffic_impl {
TETRA_HIDDEN int enqueue(tetra_rx* h, int b, hipStream_t s);
}

// A row column (COL_*) of this handle: every fetch, device view and delivery asks here whether it exists and where it lies.
namespace row_col TETRA_HIDDEN {

// TETRA_ERR_UNSUPPORTED without the column's flag, for a kind the handle does not decode, or for one that does not carry the column
inline int status(const tetra_rx* h, int col, int kind) {
    const bool flag = col == COL_BITERR ? h->biterr : col == COL_RANK ? h->list : (h->aach_rm || h->aach_soft);
    return flag && (h->kinds & (1 << kind)) && rx_out::kind_has(kind, col) ? TETRA_OK : TETRA_ERR_UNSUPPORTED;
}
// ... the same for a delivery or a bound, which name no kind: some kind of the handle has it
inline int status(const tetra_rx* h, int col) {
    for (int k = 0; k < TETRA_RX_N_KINDS; k++)
        if (status(h, col, k) == TETRA_OK) return TETRA_OK;
    return TETRA_ERR_UNSUPPORTED;
}
// where it lies: counts and ranks in buffers of their own, the distance inside the kind's rows (base is null where status is not TETRA_OK)
inline ColSrc src(const tetra_rx* h, int parity, int kind, int col) {
    const KindBufs& r = h->res[parity][kind];
    if (col == COL_BITERR) return { reinterpret_cast<const uint8_t*>(r.biterr.get()), sizeof(uint32_t) };
    if (col == COL_RANK) return { reinterpret_cast<const uint8_t*>(r.rank.get()), sizeof(int32_t) };
    return { status(h, col, kind) == TETRA_OK ? r.t2.get() + kAachDistByte : nullptr, (size_t)kKinds[kind].out_stride };
}
// the buffers of n > 0 rows that src names, for the columns this kind has (tetra_rx_create)
inline bool alloc(const tetra_rx* h, KindBufs& r, int kind, size_t n) {
    return (status(h, COL_BITERR, kind) != TETRA_OK || r.biterr.reserve(sizeof(uint32_t) * n) == hipSuccess) &&
           (status(h, COL_RANK, kind) != TETRA_OK || r.rank.reserve(sizeof(int32_t) * n) == hipSuccess);
}

}  // namespace row_col

// A per-channel table (TAB_*) of this handle, [C] elements of rx_out::chan_elem_bytes: the getters, the snapshot, the deliveries and
// the reset of single channels ask here.
namespace chan_tab TETRA_HIDDEN {

// the chain's own tables, which it zeroes and copies itself; the other two are the synchroniser's, read through its getters
inline bool own(int tab) { return tab == TAB_CELL || tab == TAB_LINK; }
// a table's element size: rx_out's for its four
inline int elem_bytes(int tab) { return tab == TAB_HANDOVER ? (int)sizeof(bsync_core::Assist) : rx_out::chan_elem_bytes(tab); }
// *p = the live table on the device, or null where the handle has none: link figures without TETRA_RX_FLAG_BITERR, miss counters
// before a tolerance was first set (TETRA_RX_FLAG_SYNC_TOLERANT sets one), the hand-over's fields before the first hand-over.  The miss counters stay when the handle returns to the
// reference's rule; *counting (may be null) is false then, which is what a reset of channels keys on -- the snapshot keys on the table.
inline int live(const tetra_rx* h, int tab, void** p, bool* counting = nullptr) {
    retune_impl::BsyncTables t = { nullptr, nullptr, true, nullptr };
    if (!own(tab)) TETRA_TRY(retune_impl::bsync_tables(h->bs, &t));
    *p = tab == TAB_CELL ? (void*)h->cell.get() : tab == TAB_LINK ? (void*)h->link.get() : tab == TAB_SYNC_STATE ? (void*)t.state
       : tab == TAB_SYNC_MISSES ? (void*)t.miss : t.assist;
    if (counting) *counting = tab != TAB_SYNC_MISSES || t.tolerant;
    return TETRA_OK;
}
// whether a snapshot can be armed with it and a delivery can carry it: TETRA_ERR_UNSUPPORTED for a table the handle does not have
inline int status(const tetra_rx* h, int tab) {
    if (tab == TAB_LINK) return h->biterr ? TETRA_OK : TETRA_ERR_UNSUPPORTED;      // (asked before the table is allocated, too)
    void* p = nullptr;
    TETRA_TRY(live(h, tab, &p));
    return p ? TETRA_OK : TETRA_ERR_UNSUPPORTED;
}

}  // namespace chan_tab
