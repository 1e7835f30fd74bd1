// traffic_core.hpp -- lane code of the traffic routing (include/ext/tetra_traffic.h): which frame slots of a call are decoded as TCH
// blocks, and how many of them are kept.  The rule is the lower MAC's side of the reference's: tp_sap_udata_ind treats the SCH/F block
// of a burst as traffic when cur_burst.is_traffic is set (tetra_lower_mac.c:287), which the upper MAC takes from the burst's own
// ACCESS-ASSIGN (tetra_upper_mac.c:499-504 behind macpdu_decode_access_assign, tetra_mac_pdu.c:257-297).  Which timeslot carries which
// kind is the host's table; nothing else of the upper MAC is here.
// Host- and device-callable (tests/emul/traffic_emul.cpp runs it on the host); no stores; one lane per frame slot.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) && !defined(TETRA_HOST_EMUL)
#define TRAFFIC_HD __host__ __device__ __forceinline__
#else
#define TRAFFIC_HD inline
#endif

namespace traffic_core {

// tetra_rx_traffic_slot_t, byte for byte
struct Slot {
    uint8_t kind, usage, pad[2];
};
constexpr int kKinds = 3, kFirstKind = 8;      // TETRA_LMAC_T_TCH_7_2 / _4_8 / _2_4 = 8, 9, 10: list k holds kind kFirstKind + k
constexpr int kTrainNorm1 = 0;                 // TETRA_TRAIN_NORM_1
constexpr int kCounts = 3;                     // per kind: rows routed, kept, dropped

// what tetra_rx_set_traffic accepts
TRAFFIC_HD bool slot_valid(Slot s) {
    return (s.kind == 0 || (s.kind >= kFirstKind && s.kind < kFirstKind + kKinds)) && (s.usage == 0 || (s.usage >= 4 && s.usage <= 63));
}

// Rule (e): the frame's BBK row -- its verdict and its first 8 bits, one per byte -- names downlink usage marker `usage`.
// macpdu_decode_access_assign with f18 = 0: header = bits 0..1, field1 = bits 2..7; header 0 gives field1 another meaning (both
// fields are access fields), every other header makes it the downlink usage marker, which is_traffic keys on.
TRAFFIC_HD bool usage_matches(int bbk_ok, const uint8_t* bbk_bits, int usage) {
    if (bbk_ok != 1) return false;
    const int hdr = (bbk_bits[0] & 1) << 1 | (bbk_bits[1] & 1);
    int field1 = 0;
    for (int i = 2; i < 8; ++i) field1 = field1 << 1 | (bbk_bits[i] & 1);
    return hdr != 0 && field1 > 3 && field1 == usage;      // (markers 1..3 are no traffic, tetra_upper_mac.c:500; the table holds none)
}

// Rules (a)..(e) for one frame slot: the list (0..2) its TCH row goes to, or -1.  slot4: the channel's four entries.  bbk_ok / bbk_bits:
// the frame's BBK row, looked at only under a gate (may be null where no entry of the channel has one).
TRAFFIC_HD int route(int frame_type, uint32_t scramb, uint32_t time, const Slot* slot4, int bbk_ok, const uint8_t* bbk_bits) {
    if (frame_type != kTrainNorm1 || scramb == 0u) return -1;
    const uint32_t tn = time & 0xffu, fn = (time >> 8) & 0xffu;
    if (tn < 1u || tn > 4u || fn == 18u) return -1;
    const Slot s = slot4[tn - 1u];
    if (s.kind < kFirstKind || s.kind >= kFirstKind + kKinds) return -1;
    if (s.usage != 0 && !usage_matches(bbk_ok, bbk_bits, s.usage)) return -1;
    return s.kind - kFirstKind;
}

// the clamp: the routed row at position pos of its list is kept (listed and decoded) iff ...
TRAFFIC_HD bool kept(int pos, int max_rows) { return pos >= 0 && pos < max_rows; }
// ... so of `routed` rows the first max_rows are -> counts[0..2] = routed, kept, dropped
TRAFFIC_HD void clamp_counts(int routed, int max_rows, int32_t* counts) {
    const int kept = routed < max_rows ? routed : max_rows;
    counts[0] = routed;
    counts[1] = kept;
    counts[2] = routed - kept;
}

}  // namespace traffic_core
