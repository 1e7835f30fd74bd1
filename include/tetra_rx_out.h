/*
 * tetra_rx_out.h -- hand-off of a receive-chain call's decoded blocks to the host in ONE asynchronous step (beside tetra_rx.h).
 *
 * tetra_rx_fetch delivers one kind at a time and blocks on every step (wait for the tail, copy the count, copy the labels, pack and
 * copy the bits).  A delivery instead gathers every selected kind of one call into ONE self-describing buffer, written by the GPU
 * straight into the destination -- page-locked host memory mapped into the GPU's address space (tetra_rx_out_host_alloc) or device
 * memory on the handle's GPU -- and returns without waiting:
 *
 *     tetra_rx_process_device(h, iq[k + 1], n, s)      the next call's demodulator runs ...
 *     tetra_rx_out_enqueue(h, 1, 0, flags, buf, cap, &call)   ... while call k's blocks are gathered into buf
 *     (one call later)  tetra_rx_out_wait(h, call)  ->  tetra_rx_out_view(buf, ...) per kind: the upper MAC consumes call k
 *
 * Layout of a delivery (all offsets from the start of the buffer, little endian):
 *   tetra_rx_out_header_t                          magic, status, flags, call index, bytes needed, per selected kind: rows, row
 *                                                  bytes, offsets.  kinds[0 .. n_kinds) in ascending kind order; the rest zero.
 *   per selected kind, in that order:
 *     tetra_rx_block_t[n_rows]   at blocks_offset  (16-byte aligned)
 *     type-1 rows [n_rows][row_bytes] at bits_offset (16-byte aligned, rows back to back)
 *       byte per bit (default): row_bytes = tetra_rx_type1_bits(kind), exactly what tetra_rx_fetch delivers
 *       TETRA_RX_OUT_PACKED:    8 bits per byte, the first bit in bit 7, each row padded with zero bits to whole bytes:
 *                               row_bytes = 8 / 4 / 16 / 16 / 16 / 34 for SB1 / BBK / SB2 / NDB1 / NDB2 / SCH-F
 * Rows are tetra_rx_fetch's rows of the same call in the same (channel, frame) order; with TETRA_RX_OUT_CRC_GOOD only the rows
 * with crc_ok != 0 are kept (order preserved), and n_rows_decoded still counts every decoded row.
 *
 * Ordering: a delivery runs on the handle's own fetch stream behind the tail of the call it reads.  The results are double buffered
 * by call parity, so the tail of call k + 2 would overwrite what a delivery of call k reads: while such a delivery is pending,
 * tetra_rx_process_device makes that tail wait for it on the device (in TETRA_RX_FLAG_ONE_STREAM mode the caller's stream waits).
 * With no delivery pending nothing changes.  The destination must stay allocated until the delivery has completed
 * (tetra_rx_out_wait, or tetra_rx_reset / tetra_rx_destroy, which synchronise the device); the caller must not read a delivery
 * before it has completed.
 *
 * Host-mapped destinations are written by the GPU over the host link; they are allocated coherent (tetra_rx_out_host_alloc), so the
 * bytes are visible to the host once tetra_rx_out_query returns 0 or tetra_rx_out_wait returns.
 */
#ifndef TETRA_RX_OUT_H
#define TETRA_RX_OUT_H

#include <stddef.h>
#include <stdint.h>

#include "tetra_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    TETRA_RX_OUT_PACKED = 1,      /* type-1 bits 8 per byte (first bit in bit 7), rows padded to whole bytes */
    TETRA_RX_OUT_CRC_GOOD = 2     /* keep only the rows with crc_ok != 0 */
};

#define TETRA_RX_OUT_MAGIC 0x4f585254u     /* "TRXO" */

typedef struct tetra_rx_out_kind {
    int32_t kind;                 /* TETRA_RX_KIND_* */
    int32_t n_rows;               /* rows in this delivery */
    int32_t n_rows_decoded;       /* rows the call decoded (= n_rows without TETRA_RX_OUT_CRC_GOOD) */
    int32_t row_bytes;            /* bytes per type-1 row */
    uint64_t blocks_offset;       /* tetra_rx_block_t[n_rows] */
    uint64_t bits_offset;         /* uint8_t[n_rows][row_bytes] */
} tetra_rx_out_kind_t;

typedef struct tetra_rx_out_header {
    uint32_t magic;               /* TETRA_RX_OUT_MAGIC */
    int32_t status;               /* TETRA_OK, or TETRA_ERR_SIZE: the delivery did not fit; only this header was written */
    int32_t flags;                /* TETRA_RX_OUT_* */
    int32_t n_kinds;              /* entries of kinds[] in use */
    int64_t call;                 /* 0-based index of the process call (counted from create / the last reset) */
    uint64_t bytes;               /* bytes the whole delivery needs (also on TETRA_ERR_SIZE) */
    tetra_rx_out_kind_t kinds[TETRA_RX_N_KINDS];
} tetra_rx_out_header_t;

/* Bytes a delivery of `kinds` (bit mask of 1 << TETRA_RX_KIND_*, 0 = every kind the handle decodes) with `flags` can need at most:
 * every frame slot of a call one burst type, the worst of the three, plus the alignment padding.  Host only, no GPU work.
 * TETRA_ERR_UNSUPPORTED for a kind the configuration does not decode. */
int tetra_rx_out_bound(tetra_rx_t* h, int kinds, int flags, uint64_t* bytes);
/*
 * Enqueue a delivery of the latest (which = 0) or the previous (which = 1) process call; returns without waiting.
 *   dst       page-locked host memory (tetra_rx_out_host_alloc, or any hipHostMalloc'd / registered memory the handle's GPU can
 *             map) or device memory on the handle's GPU.  Pageable memory or a pointer on another GPU: TETRA_ERR_ARG.
 *   capacity  bytes at dst; less than sizeof(tetra_rx_out_header_t): TETRA_ERR_SIZE here.  Nothing is written outside
 *             [dst, dst + capacity): a delivery that does not fit writes only the header (status TETRA_ERR_SIZE, bytes = what it
 *             needs) and leaves the rows on the device, where tetra_rx_fetch still finds them.
 *   *call     the 0-based index of the delivered call, for tetra_rx_out_query / _wait.  May be NULL.
 * No such call yet (which = 1 before the second call): TETRA_ERR_ARG.
 */
int tetra_rx_out_enqueue(tetra_rx_t* h, int which, int kinds, int flags, void* dst, uint64_t capacity, int64_t* call);
/* 0: every delivery of that call enqueued so far has completed; 1: pending; < 0: a status (TETRA_ERR_ARG: no delivery of that
 * call was enqueued).  The delivery's own outcome is the header's status.  The handle remembers its latest 8 deliveries; for an
 * older call the answer is that of the oldest of them (deliveries run in order, so it is never early). */
int tetra_rx_out_query(tetra_rx_t* h, int64_t call);
/* Blocks until the deliveries of that call have completed; statuses as tetra_rx_out_query. */
int tetra_rx_out_wait(tetra_rx_t* h, int64_t call);
/* Page-locked, coherent host memory mapped for every GPU; NULL on failure.  Free with tetra_rx_out_host_free. */
void* tetra_rx_out_host_alloc(size_t bytes);
void tetra_rx_out_host_free(void* p);

/* Host only (no GPU): one kind's rows of a completed delivery in host memory.  Checks the buffer before it reads it: a buffer
 * shorter than the header or than header.bytes, a wrong magic, offsets or rows outside the buffer, or a row_bytes that does not
 * match the kind and flags are TETRA_ERR_ARG; a header status other than TETRA_OK is returned as it is; a kind the delivery does
 * not hold is TETRA_ERR_UNSUPPORTED.  Any out pointer may be NULL. */
int tetra_rx_out_view(const void* buf, uint64_t bytes, int kind, const tetra_rx_block_t** blocks, const uint8_t** bits, int* n_rows,
                      int* row_bytes);
/* Host only: packed rows [n_rows][row_bytes] (first bit in bit 7) -> out [n_rows][out_stride], one bit (0 / 1) per byte, the first
 * n_bits of each row.  TETRA_ERR_ARG: NULL with n_rows > 0, negative counts, n_bits > 8 * row_bytes; TETRA_ERR_SIZE:
 * out_stride < n_bits. */
int tetra_rx_unpack_bits(const uint8_t* packed, int n_rows, int row_bytes, int n_bits, uint8_t* out, int out_stride);

#ifdef __cplusplus
}
#endif
#endif
