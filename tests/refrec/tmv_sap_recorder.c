/* Test-side recorder BELOW the reference's lower MAC: what lower_mac/tetra_lower_mac.c needs from downstream, so that the
 * reference's own tp_sap_udata_ind() -- the SYNC-PDU read-out into tcd, the copy of tcd->time to and from t_phy_state.time, the
 * scrambling code every later block is descrambled with -- can RUN in the tests, behind the reference's own tetra_burst_sync_in()
 * and tetra_burst_rx_cb().  oracle/build_ref.sh links it with the reference's sources, compiled where they lie, into
 * oracle/_ref/libtetra_rxchain_ref.so (-Bsymbolic: the library calls its own tp_sap_udata_ind and uses its own t_phy_state whatever
 * else the process has loaded).
 *
 * Our own code (nothing copied).  It defines
 *   upper_mac_prim_recv       one event per TMV-SAP unitdata indication; returns -1 ("done with this block")
 *   update_current_network    stores the two numbers
 *   the five ETSI codec entry points (prototypes: standin/c-code/)   abort(): reachable only with is_traffic set, which no test sets
 * and owns the structs the reference's functions want, so that no struct layout is restated in Python.  tcd is a static of the
 * reference's file and t_phy_state a global: a fresh receiver is a fresh private copy of the library (oracle/ref_binding.py).
 * Test infrastructure only. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <tetra_common.h>
#include <tetra_tdma.h>
#include <tetra_prim.h>
#include <phy/tetra_burst.h>
#include <phy/tetra_burst_sync.h>
#include <crypto/tetra_crypto.h>
#include "tetra_upper_mac.h"

#include "c-code/channel.h"
#include "c-code/source.h"

extern struct tetra_phy_state t_phy_state;

typedef struct {
    int32_t lchan, blk_num, crc_ok, n_bits;   /* tup->lchan / blk_num / crc_ok; type-1 bits at msg->l1h */
    uint32_t scrambling_code;                 /* tup->scrambling_code */
    uint32_t tup_tn, tup_fn, tup_mn;          /* tup->tdma_time */
    uint32_t phy_tn, phy_fn, phy_mn;          /* t_phy_state.time when the indication arrives */
    uint32_t bitbuf_start_bitnum;             /* the receiver's, i.e. the bit number of the frame being handed over */
    int32_t rx_state;                         /* the receiver's state (enum rx_state) */
    int32_t curr_frame, curr_multiframe;      /* t_display_st's, stored by tetra_burst_rx_cb on entry */
    uint8_t bits[268];
} rxc_event_t;

typedef struct {
    struct tetra_rx_state rx;
    struct tetra_mac_state mac;
    struct tetra_display_state disp;
    struct tetra_crypto_state tcs;
    int network_updates;
    rxc_event_t* ev;
    int n_ev, cap_ev;
} rxc_t;

int upper_mac_prim_recv(struct osmo_prim_hdr* op, void* priv) {
    rxc_t* r = (rxc_t*)((char*)priv - offsetof(rxc_t, mac));
    const struct tetra_tmvsap_prim* tmvp = (const struct tetra_tmvsap_prim*)op;      /* oph is its first member */
    const struct tmv_unitdata_param* tup = &tmvp->u.unitdata;
    const struct msgb* msg = op->msg;
    if (r->n_ev == r->cap_ev) {
        r->cap_ev = r->cap_ev ? 2 * r->cap_ev : 256;
        r->ev = (rxc_event_t*)realloc(r->ev, sizeof(rxc_event_t) * (size_t)r->cap_ev);
    }
    rxc_event_t* e = &r->ev[r->n_ev++];
    memset(e, 0, sizeof(*e));
    e->lchan = (int32_t)tup->lchan;
    e->blk_num = tup->blk_num;
    e->crc_ok = tup->crc_ok;
    e->scrambling_code = tup->scrambling_code;
    e->tup_tn = tup->tdma_time.tn; e->tup_fn = tup->tdma_time.fn; e->tup_mn = tup->tdma_time.mn;
    e->phy_tn = t_phy_state.time.tn; e->phy_fn = t_phy_state.time.fn; e->phy_mn = t_phy_state.time.mn;
    e->bitbuf_start_bitnum = r->rx.bitbuf_start_bitnum;
    e->rx_state = (int32_t)r->rx.state;
    e->curr_frame = r->disp.curr_frame;
    e->curr_multiframe = r->disp.curr_multiframe;
    const unsigned n = msgb_l1len(msg);
    e->n_bits = (int32_t)n;
    memcpy(e->bits, msg->l1h, n <= sizeof(e->bits) ? n : sizeof(e->bits));
    return -1;
}

void update_current_network(struct tetra_crypto_state* tcs, int mcc, int mnc) {
    rxc_t* r = (rxc_t*)((char*)tcs - offsetof(rxc_t, tcs));
    tcs->mcc = (uint32_t)mcc;
    tcs->mnc = (uint32_t)mnc;
    r->network_updates++;
}

int16_t Desinterleaving_Speech(int16_t interleaved[], int16_t coded[]) { (void)interleaved; (void)coded; abort(); }
int16_t Channel_Decoding(int16_t first_pass, int16_t frame_stealing, int16_t coded[], int16_t reordered[]) {
    (void)first_pass; (void)frame_stealing; (void)coded; (void)reordered; abort();
}
void Bits2prm_Tetra(int16_t serial[], int16_t parm[]) { (void)serial; (void)parm; abort(); }
void Decod_Tetra(int16_t parm[], int16_t synth[]) { (void)parm; (void)synth; abort(); }
void Post_Process(int16_t synth[], int16_t length) { (void)synth; (void)length; abort(); }

rxc_t* rxc_new(void) {
    rxc_t* r = (rxc_t*)calloc(1, sizeof(rxc_t));
    r->mac.t_display_st = &r->disp;
    r->mac.tcs = &r->tcs;
    r->rx.burst_cb_priv = &r->mac;
    return r;
}

void rxc_free(rxc_t* r) {
    if (r) { free(r->ev); free(r); }
}

/* bits -> the reference's tetra_burst_sync_in, `chunk` bits per call */
void rxc_feed(rxc_t* r, const uint8_t* bits, int n_bits, int chunk) {
    uint8_t tmp[4096];
    if (chunk < 1) chunk = 1;
    if (chunk > (int)sizeof(tmp)) chunk = (int)sizeof(tmp);
    for (int i = 0; i < n_bits; i += chunk) {
        const int n = n_bits - i < chunk ? n_bits - i : chunk;
        memcpy(tmp, bits + i, (size_t)n);       /* the reference takes a non-const pointer */
        tetra_burst_sync_in(&r->rx, tmp, (unsigned)n);
    }
}

/* one block straight into the reference's tp_sap_udata_ind, as tetra_burst_rx_cb would hand it over */
void rxc_udata_ind(rxc_t* r, int type, int blk_num, const uint8_t* bits, int len) {
    tp_sap_udata_ind((enum tp_sap_data_type)type, blk_num, bits, (unsigned)len, &r->mac);
}

/* the LOCKED receiver's per-frame clock step (tetra_burst_sync.c:113) */
void rxc_add_tn(int count) { tetra_tdma_time_add_tn(&t_phy_state.time, (uint32_t)count); }
void rxc_get_phy_time(uint32_t out[3]) { out[0] = t_phy_state.time.tn; out[1] = t_phy_state.time.fn; out[2] = t_phy_state.time.mn; }
void rxc_set_phy_time(uint32_t tn, uint32_t fn, uint32_t mn) { t_phy_state.time.tn = tn; t_phy_state.time.fn = fn; t_phy_state.time.mn = mn; }
/* where this copy of the library keeps its callback and its clock (the test that shows the library is self-contained) */
const void* rxc_own_udata_ind(void) { return (const void*)tp_sap_udata_ind; }
const void* rxc_own_phy_state(void) { return &t_phy_state; }

/* (mcc, mnc) as update_current_network last stored them, the colour code tp_sap_udata_ind left in tcs->cc, the number of updates */
void rxc_network(const rxc_t* r, int32_t out[4]) {
    out[0] = (int32_t)r->tcs.mcc; out[1] = (int32_t)r->tcs.mnc; out[2] = r->tcs.cc; out[3] = r->network_updates;
}

/* rx state as four words (state, bits_in_buf, bitbuf_start_bitnum, next_frame_start_bitnum) */
void rxc_rx_state(const rxc_t* r, uint32_t out[4]) {
    out[0] = (uint32_t)r->rx.state;
    out[1] = r->rx.bits_in_buf;
    out[2] = r->rx.bitbuf_start_bitnum;
    out[3] = r->rx.next_frame_start_bitnum;
}

int rxc_event_count(const rxc_t* r) { return r->n_ev; }
int rxc_event_size(void) { return (int)sizeof(rxc_event_t); }
void rxc_events(const rxc_t* r, int first, int count, rxc_event_t* out) { memcpy(out, r->ev + first, sizeof(rxc_event_t) * (size_t)count); }
void rxc_clear_events(rxc_t* r) { r->n_ev = 0; }
