/*
 * tetra_rx_out_ext.h -- the opt-in results of a receive-chain call through the one-step delivery (beside tetra_rx_out.h).
 *
 * A delivery (tetra_rx_out.h) carries a call's labels and type-1 rows.  The chain's opt-in features compute more: per coded row the
 * channel bit-error count (tetra_biterr.h) and the list-decoding rank (tetra_list.h), per BBK row the Reed-Muller distance
 * (tetra_aach.h), and per channel the cell state, the synchroniser's state and miss counter (tetra_sync_tol.h) and the link figures
 * (tetra_biterr.h).  The entry points declared here deliver them WITH the rows: same buffer, same asynchronous step, no host
 * synchronisation, and -- unlike the blocking getters, which answer with the state behind the latest tail -- the per-channel state of
 * the call the delivery belongs to.  tetra_rx_out.h keeps its declarations, its format and its device code; with extras = 0 the entry
 * points here enqueue what tetra_rx_out_enqueue enqueues and write the same bytes.
 *
 * Layout of an extended delivery.  The classic delivery is written unchanged: header, labels, bits, header.bytes = the classic size,
 * and tetra_rx_out_view reads it as ever.  Behind it, at align16(header.bytes), sits the extension block (all offsets from the start
 * of the buffer, little endian, every section 16-byte aligned, 0 = the section is absent):
 *   tetra_rx_out_ext_header_t    magic, the extras delivered, call index, n_channels, bytes of the WHOLE buffer contents, per selected
 *                                kind (the classic header's kinds[], same order) the offsets of its columns, the offsets of the
 *                                per-channel tables
 *   per selected kind, in that order, the columns it has, each [n_rows] in exactly the delivered rows' order (entry r belongs to
 *   label r; with TETRA_RX_OUT_CRC_GOOD compacted like the rows):
 *     uint32 biterr[n_rows]      TETRA_RX_OUT_EXT_ROW_BITERR, coded kinds: tetra_rx_fetch_biterr's value (errors | compared << 16)
 *     int32  rank[n_rows]        TETRA_RX_OUT_EXT_ROW_LIST_RANK, coded kinds: tetra_rx_fetch_list_rank's value
 *     uint8  aach_dist[n_rows]   TETRA_RX_OUT_EXT_ROW_AACH_DIST, BBK: tetra_rx_fetch_aach_dist's value
 *   per-channel tables [n_channels], in this order:
 *     tetra_lmac_cell_state_t    TETRA_RX_OUT_EXT_CHAN_CELL
 *     tetra_bsync_state_t        TETRA_RX_OUT_EXT_CHAN_SYNC_STATE
 *     int32 misses               TETRA_RX_OUT_EXT_CHAN_SYNC_MISSES
 *     tetra_rx_link_t            TETRA_RX_OUT_EXT_CHAN_LINK
 * A row extra applies to the selected kinds that have it; a delivery that selects none of them has no such column, and the bit is
 * not set in the extension header's extras.
 *
 * If classic part plus extension do not fit the capacity, only the classic header is written: status TETRA_ERR_SIZE, bytes = the
 * TOTAL needed (classic part, padding and extension), nothing past the header.
 *
 * Per-channel state of the right call.  Cell, synchroniser, miss and link state exist once per handle, and the tail of call k + 1 may
 * run while call k's delivery is read.  tetra_rx_out_set_snapshot arms a mask of channel extras: from the next process call on, every
 * tail ends with one small kernel that copies the armed tables into a snapshot, double buffered by call parity like the results, and
 * a delivery reads the snapshot of its call.  A snapshot is the state AS CALL k'S TAIL LEFT IT: tetra_rx_reset_channels_device and
 * tetra_wbrx_retune, which change channels between calls, do not touch it.  With mask 0 (the default) the tail launches what it
 * always launched.  The copy runs behind the link figures' kernel and outside the spans tetra_rx_stage_ms reports.
 * Same conventions as tetra_rx_out.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions.
 */
#ifndef TETRA_RX_OUT_EXT_H
#define TETRA_RX_OUT_EXT_H

#include <stdint.h>

#include "../tetra_burst_sync.h"
#include "../tetra_lmac.h"
#include "../tetra_rx.h"
#include "../tetra_rx_out.h"
#include "tetra_biterr.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    TETRA_RX_OUT_EXT_ROW_BITERR = 1,          /* needs TETRA_RX_FLAG_BITERR */
    TETRA_RX_OUT_EXT_ROW_LIST_RANK = 2,       /* needs TETRA_RX_FLAG_LIST */
    TETRA_RX_OUT_EXT_ROW_AACH_DIST = 4,       /* needs TETRA_RX_FLAG_AACH_RM3014 and a handle that decodes BBK */
    TETRA_RX_OUT_EXT_CHAN_CELL = 16,
    TETRA_RX_OUT_EXT_CHAN_SYNC_STATE = 32,
    TETRA_RX_OUT_EXT_CHAN_SYNC_MISSES = 64,   /* needs TETRA_RX_FLAG_SYNC_TOLERANT or a tolerance set (tetra_rx_set_sync_tolerance) */
    TETRA_RX_OUT_EXT_CHAN_LINK = 128          /* needs TETRA_RX_FLAG_BITERR */
};
#define TETRA_RX_OUT_EXT_ROW_ALL 7
#define TETRA_RX_OUT_EXT_CHAN_ALL 240

#define TETRA_RX_OUT_EXT_MAGIC 0x58585254u    /* "TRXX" */

typedef struct tetra_rx_out_ext_kind {
    int32_t kind;                 /* TETRA_RX_KIND_*, = the classic header's kinds[i].kind */
    int32_t n_rows;               /* = the classic header's kinds[i].n_rows */
    uint64_t biterr_offset;       /* uint32_t[n_rows], 0 = absent */
    uint64_t rank_offset;         /* int32_t[n_rows], 0 = absent */
    uint64_t aach_dist_offset;    /* uint8_t[n_rows], 0 = absent */
} tetra_rx_out_ext_kind_t;

typedef struct tetra_rx_out_ext_header {
    uint32_t magic;               /* TETRA_RX_OUT_EXT_MAGIC */
    int32_t extras;               /* TETRA_RX_OUT_EXT_* actually delivered */
    int64_t call;                 /* = the classic header's call */
    int32_t n_channels;           /* entries of each per-channel table */
    int32_t n_kinds;              /* = the classic header's n_kinds */
    uint64_t bytes;               /* bytes of the whole buffer contents: classic part, padding, this block */
    uint64_t cell_offset;         /* tetra_lmac_cell_state_t[n_channels], 0 = absent */
    uint64_t sync_state_offset;   /* tetra_bsync_state_t[n_channels], 0 = absent */
    uint64_t sync_misses_offset;  /* int32_t[n_channels], 0 = absent */
    uint64_t link_offset;         /* tetra_rx_link_t[n_channels], 0 = absent */
    tetra_rx_out_ext_kind_t kinds[TETRA_RX_N_KINDS];
} tetra_rx_out_ext_header_t;

/* Bytes an extended delivery of `kinds` with `flags` and `extras` can need at most: tetra_rx_out_bound's worst case plus the
 * extension block for the same rows.  Host only, no GPU work.  Statuses as tetra_rx_out_enqueue_ext's argument checks. */
int tetra_rx_out_bound_ext(tetra_rx_t* h, int kinds, int flags, int extras, uint64_t* bytes);
/*
 * tetra_rx_out_enqueue with `extras` (TETRA_RX_OUT_EXT_*), a mask of its own: it never enters tetra_rx_out_header_t.flags.
 * Every other argument, the ordering and tetra_rx_out_query / _wait as there.  extras = 0: exactly tetra_rx_out_enqueue.
 *   an unknown bit:                                      TETRA_ERR_ARG
 *   an extra whose flag the handle was created without:  TETRA_ERR_UNSUPPORTED, as its blocking fetch answers
 *   a channel extra of a call whose tail took no such snapshot (tetra_rx_out_set_snapshot not armed with it when that call was
 *   processed -- armed later included):                  TETRA_ERR_ARG
 * A row extra none of the selected kinds has is not an error.
 */
int tetra_rx_out_enqueue_ext(tetra_rx_t* h, int which, int kinds, int flags, int extras, void* dst, uint64_t capacity, int64_t* call);
/* Arms (or, with 0, disarms) the per-call snapshot of the channel extras in `chan_extras`, from the next process call on.  Enqueues
 * nothing and waits for nothing (the first arming allocates the two snapshots): callable at any time.  A bit outside TETRA_RX_OUT_EXT_CHAN_ALL: TETRA_ERR_ARG; one whose flag the handle lacks: TETRA_ERR_UNSUPPORTED.
 * tetra_rx_reset keeps the mask and invalidates the snapshots taken so far. */
int tetra_rx_out_set_snapshot(tetra_rx_t* h, int chan_extras);

/* Host only (no GPU): one kind's columns of a completed extended delivery in host memory; a column the delivery does not hold comes
 * back NULL.  Checks the buffer before it reads it, like tetra_rx_out_view (whose statuses for the classic part it returns): the
 * extension's magic, call and kinds against the classic header's, every offset inside the extension's bytes (which are inside the
 * buffer) and 16-byte aligned, n_rows equal to the classic entry's: else TETRA_ERR_ARG.  A buffer that ends before an extension
 * header could: TETRA_ERR_UNSUPPORTED.  Any out pointer may be NULL. */
int tetra_rx_out_view_ext(const void* buf, uint64_t bytes, int kind, const uint32_t** biterr, const int32_t** rank, const uint8_t** aach_dist,
                          int* n_rows);
/* Host only: the per-channel tables, checked the same way; a table the delivery does not hold comes back NULL. */
int tetra_rx_out_view_channels(const void* buf, uint64_t bytes, const tetra_lmac_cell_state_t** cell, const tetra_bsync_state_t** sync,
                               const int32_t** misses, const tetra_rx_link_t** link, int* n_channels);

#ifdef __cplusplus
}
#endif
#endif
