/*
 * tetra_traffic.h -- the receive chain decodes the traffic slots the host names as TCH blocks.  OPT-IN: a handle that never calls
 * tetra_rx_traffic_enable allocates, launches and computes exactly what it does without this header.
 *
 * The reference's lower MAC treats the SCH/F block of a burst as traffic when its upper MAC has set cur_burst.is_traffic
 * (src/decoder/src/lower_mac/tetra_lower_mac.c:287), which that takes from the burst's own ACCESS-ASSIGN
 * (upper_mac/tetra_upper_mac.c:499-504).  Which (channel, timeslot) carries circuit-mode data, and at which rate, is upper-MAC knowledge
 * and stays with the host: it is handed in as a table.  The device applies the lower MAC's side of the rule only.
 *
 * The table: per channel tetra_rx_traffic_slot_t slot[4], one entry per timeslot 1..4.
 *     kind    0 (off, the default) or TETRA_LMAC_T_TCH_7_2 / _4_8 / _2_4 (tetra_tch.h)
 *     usage   0 (no gate) or the expected downlink usage marker 4..63
 * Frame slot r of channel c of a call yields one TCH row of kind K iff (csrc/traffic_core.hpp, the one place the rule is written)
 *   (a) its burst type is TETRA_TRAIN_NORM_1 -- a NORM_2 burst in a traffic slot is a stolen slot and stays the NDB 1 / 2 rows it is;
 *   (b) the scrambling code in force for it is not 0: the channel has had a SYNC PDU with a good CRC (every cell's code has its low
 *       bits set, so 0 means "fresh receiver");
 *   (c) its TDMA time t (the label's tdma_time) has tn = t & 0xff in 1..4 and fn = (t >> 8) & 0xff other than 18;
 *   (d) slot[tn - 1].kind == K;
 *   (e) if slot[tn - 1].usage != 0: the BBK row of the same frame has crc_ok == 1, its header bits[0] << 1 | bits[1] is not 0, and
 *       field1 (bits 2..7, first bit most significant) equals usage -- macpdu_decode_access_assign with f18 = 0
 *       (tetra_mac_pdu.c:257-297) followed by tetra_upper_mac.c:499-504, restricted to one equality.  Under TETRA_RX_FLAG_AACH_RM3014 /
 *       _AACH_SOFT the gate reads the corrected row and that decoder's verdict.
 * The routed frame's rows of the six kinds of tetra_rx.h are what they are without this header: its SCH/F row is still delivered,
 * CRC-bad, as the reference does too.  The TCH rows are decoded as tetra_tch.h defines them (N = 1), from the packed frames; with
 * TETRA_RX_FLAG_SOFT TCH/4.8 and TCH/2.4 from the soft ring (tetra_tch_soft.h) and TCH/7.2, which is not coded, from the packed frames
 * still.  With TETRA_RX_FLAG_BITERR the two coded kinds carry their errors | compared << 16 words; the link figures stay over the
 * signalling kinds.  TETRA_RX_FLAG_LIST does nothing here: there is no CRC.
 *
 * The routing and the decode run on the tail's stream behind the link figures, outside the spans of tetra_rx_stage_ms and in front of
 * the tail's event: a fetch that waits for the tail sees the traffic rows.  A kind's rows are in (channel, frame) order.
 *
 * Memory, allocated by tetra_rx_traffic_enable for max_rows rows per TCH kind, twice (two calls): 432 + 296 + 152 bytes of rows,
 * 3 x 24 of labels, 3 x 4 of verdicts and 3 x 4 of frame indices -- 976 bytes per row and call, 1952 in all; TETRA_RX_FLAG_BITERR adds
 * 2 x 4 per call.  The decoder's decision scratch: 896 bytes per row (in whole groups of 64 rows), once.  The table: 16 bytes per channel.
 *
 * The table is configuration: no reset, retune, hand-over or gap clears it.  A restarted channel routes nothing until its next SYNC
 * PDU with a good CRC, by rule (b).
 *
 * Out of scope: interleaving over N = 4 / 8 blocks inside the chain (tetra_tch_nblk.h works on a pool of bursts that would have to
 * survive calls); speech (TCH/S); traffic rows in the one-step delivery of tetra_rx_out.h; any ACCESS-ASSIGN parsing beyond (e).
 * Same conventions as tetra_rx.h: extern "C", int status (TETRA_OK / TETRA_ERR_*), no exceptions, GPU only.
 */
#ifndef TETRA_TRAFFIC_H
#define TETRA_TRAFFIC_H

#include <stdint.h>

#include "../tetra_rx.h"
#include "tetra_tch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tetra_rx_traffic_slot {
    uint8_t kind;                  /* 0 or TETRA_LMAC_T_TCH_* */
    uint8_t usage;                 /* 0 or 4..63 */
    uint8_t pad[2];                /* ignored on the way in, zero on the way out */
} tetra_rx_traffic_slot_t;

/* Row strides of the three kinds on the device (tetra_rx_traffic_rows_device), type-2 bits first: 432 / 296 / 152. */
#define TETRA_RX_TRAFFIC_STRIDE(tch_kind) ((tch_kind) == TETRA_LMAC_T_TCH_7_2 ? 432 : (tch_kind) == TETRA_LMAC_T_TCH_4_8 ? 296 : 152)

/*
 * Once per handle; synchronises the device.  max_rows in 1 .. tetra_rx_max_rows(h): the most rows per TCH kind and call that are
 * kept (the first max_rows in (channel, frame) order; the rest are counted as dropped).  The table starts all zero: nothing routed.
 * A second call is TETRA_ERR_ARG.  Until this call every other function below returns TETRA_ERR_UNSUPPORTED.  Allowed on a chain
 * owned by a wideband handle (tetra_wbrx_rx).
 */
int tetra_rx_traffic_enable(tetra_rx_t* h, int max_rows);

/*
 * The entries of channels [first, first + count) from host memory, slots [count][4].  Stream-ordered, no host synchronisation: the
 * entries are copied at once into a page-locked staging block (the call may return before the device has read them) and reach the
 * table on hip_stream behind the tail of every tetra_rx_process* call enqueued so far; the next tetra_rx_process* call waits for
 * them on the device.  So a call already enqueued is decoded with the table it was enqueued under, and the next one with this.
 * TETRA_ERR_ARG: a kind other than 0 / TETRA_LMAC_T_TCH_*, a usage of 1..3 or above 63, or a usage on a handle whose kinds leave
 * TETRA_RX_KIND_BBK out -- nothing is changed then.
 */
int tetra_rx_set_traffic(tetra_rx_t* h, int first, int count, const tetra_rx_traffic_slot_t* slots, void* hip_stream);

/* The table as the latest tetra_rx_set_traffic leaves it, read back from the device (waits for that upload). */
int tetra_rx_get_traffic(tetra_rx_t* h, int first, int count, tetra_rx_traffic_slot_t* slots);

/*
 * tetra_rx_fetch for the rows of one TCH kind of call `which` (0 = latest, 1 = the one before): waits for that call's tail.
 *   blocks     [capacity] labels, may be NULL (crc_ok = 1: there is nothing to check)
 *   type2      [capacity][stride] uint8 host, one bit per byte, may be NULL: the kind's type-2 bits (432 / 292 / 148, of which the
 *              first 432 / 288 / 144 are type-1); stride below that is TETRA_ERR_SIZE
 *   biterr     [capacity] uint32, may be NULL: errors | compared << 16 (tetra_biterr.h); TETRA_ERR_UNSUPPORTED if given on a handle
 *              without TETRA_RX_FLAG_BITERR or for TETRA_LMAC_T_TCH_7_2
 *   n_rows     the rows kept (at most max_rows); more than capacity with an output pointer given is TETRA_ERR_SIZE
 *   n_dropped  may be NULL: the rows routed beyond max_rows, which were not decoded
 * No such call yet: no rows, TETRA_OK.
 */
int tetra_rx_fetch_traffic(tetra_rx_t* h, int which, int tch_kind, tetra_rx_block_t* blocks, uint8_t* type2, int stride, int capacity,
                           uint32_t* biterr, int* n_rows, int* n_dropped);

/*
 * tetra_rx_rows_device for one TCH kind: the rows where they lie, hip_stream made to wait for the call's tail.  Every output may be
 * NULL.  d_counts: int32 [3] = rows routed, rows kept (the rows present), rows dropped.  d_biterr: NULL without the flag or for TCH/7.2.
 */
int tetra_rx_traffic_rows_device(tetra_rx_t* h, int which, int tch_kind, const uint8_t** d_type2, int* type2_stride,
                                 const tetra_rx_block_t** d_blocks, const int32_t** d_counts, const uint32_t** d_biterr, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif
