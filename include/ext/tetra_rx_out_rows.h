/*
 * tetra_rx_out_rows.h -- the one-step delivery (tetra_rx_out.h, ext/tetra_rx_out_ext.h) over rows the CALLER provides.
 *
 * tetra_rx_out_enqueue gathers a receive-chain call's decoded rows into one self-describing buffer; the rows, their CRC verdicts and
 * their count are the handle's.  The entry point declared here is the same launch for a caller that has rows of its own on the device
 * -- a decoder driven by hand (tetra_lmac.h), a test that plants rows -- with no handle: the chain and this entry share one launch
 * function, the kernels and the format are tetra_rx_out.h's, and the buffer reads with tetra_rx_out_view / tetra_rx_out_view_ext.
 * Same conventions as tetra_rx_out.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only, the current device.
 */
#ifndef TETRA_RX_OUT_ROWS_H
#define TETRA_RX_OUT_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include "../tetra_rx.h"
#include "../tetra_rx_out.h"
#include "tetra_rx_out_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One kind's rows on the device, as the chain's decoder leaves them. */
typedef struct tetra_rx_out_rows {
    int32_t kind;                      /* TETRA_RX_KIND_*; the array is in ascending kind order, no kind twice */
    int32_t type2_stride;              /* bytes from row to row: a multiple of 8, >= 8 * ceil(type1_bits / 8) (BBK: >= 32) */
    const uint8_t* d_type2;            /* [max_rows][type2_stride], 8-byte aligned; type-1 bits first, one 0/1 byte per bit */
    const int32_t* d_crc_ok;           /* [max_rows]; TETRA_RX_OUT_CRC_GOOD keeps the rows whose entry is not 0 */
    const tetra_rx_block_t* d_blocks;  /* [max_rows], 8-byte aligned; delivered as they are (their crc_ok field is not looked at) */
    const int32_t* d_n_rows;           /* [1] on the device; clamped to 0..max_rows as the chain does */
    const uint32_t* d_biterr;          /* [max_rows] or NULL: the TETRA_RX_OUT_EXT_ROW_BITERR column of a coded kind */
    const int32_t* d_rank;             /* [max_rows] or NULL: the TETRA_RX_OUT_EXT_ROW_LIST_RANK column of a coded kind */
} tetra_rx_out_rows_t;

/* Bytes of device scratch a launch over up to max_rows rows per kind needs: the kept rows per tile of 128 rows
 * ([TETRA_RX_N_KINDS][ceil(max_rows / 128)] ints) and the two layouts the write launches read.  0 for max_rows < 1. */
size_t tetra_rx_out_rows_workspace_bytes(int max_rows);
/*
 * Enqueues on hip_stream the launches of tetra_rx_out_enqueue (row_extras = 0: exactly those) or tetra_rx_out_enqueue_ext over the
 * rows of kinds[0 .. n_kinds) and returns without synchronising; every array must stay valid and unchanged until that work is done.
 *   flags        TETRA_RX_OUT_PACKED | TETRA_RX_OUT_CRC_GOOD
 *   row_extras   a subset of TETRA_RX_OUT_EXT_ROW_ALL.  Not 0: the extension block follows the classic part, with n_channels = 0 and
 *                no per-channel table.  ROW_BITERR / ROW_LIST_RANK deliver d_biterr / d_rank of the coded kinds, ROW_AACH_DIST byte 30
 *                of every BBK row, as the chain does.
 *   call         the call index written into the header(s)
 *   dst, capacity  as tetra_rx_out_enqueue's: page-locked host memory the current GPU can map or device memory on the current GPU,
 *                16-byte aligned.  Nothing is written outside [dst, dst + capacity): a delivery that does not fit writes only the
 *                classic header (status TETRA_ERR_SIZE, bytes = what the whole needs).
 *   d_workspace  tetra_rx_out_rows_workspace_bytes(max_rows) bytes on the device, 16-byte aligned; the launch's alone until its work on
 *                the stream is done (launches on ONE stream may share it: they run one after the other).  Its contents do not matter.
 * Of a kind's arrays only the rows below min(*d_n_rows, max_rows) are read; a column the kind does not carry (counts and ranks of the
 * BBK) or that row_extras does not ask for may be NULL.
 * Statuses; but for the last, nothing is launched or written:
 *   TETRA_ERR_ARG     kinds, dst or d_workspace NULL; n_kinds outside 1..TETRA_RX_N_KINDS; max_rows < 1; a bit outside the two flags;
 *                     a bit outside TETRA_RX_OUT_EXT_ROW_ALL in row_extras (the channel extras are a handle's); a kind outside
 *                     0..TETRA_RX_N_KINDS - 1 or not above the entry before it; d_type2, d_crc_ok, d_blocks or d_n_rows NULL; a
 *                     type2_stride below the kind's minimum; a coded kind without d_biterr under ROW_BITERR or without d_rank under
 *                     ROW_LIST_RANK; dst pageable memory or memory of another GPU
 *   TETRA_ERR_ALIGN   dst or d_workspace off the 16-byte grid; d_type2 or d_blocks off the 8-byte grid; d_crc_ok, d_n_rows, d_biterr
 *                     or d_rank off the 4-byte grid; a type2_stride that is no multiple of 8
 *   TETRA_ERR_SIZE    capacity < sizeof(tetra_rx_out_header_t); workspace_bytes < tetra_rx_out_rows_workspace_bytes(max_rows)
 *   TETRA_ERR_NO_DEVICE  no current HIP device
 *   TETRA_ERR_HIP     a launch failed
 */
int tetra_rx_out_write_rows_device(const tetra_rx_out_rows_t* kinds, int n_kinds, int max_rows, int flags, int row_extras,
                                   int64_t call, void* dst, uint64_t capacity, void* d_workspace, size_t workspace_bytes,
                                   void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
