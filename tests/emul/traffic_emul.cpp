// traffic_emul.cpp -- host build of the traffic routing's lane code (csrc/traffic_core.hpp, include/ext/tetra_traffic.h): the rule per
// entry, and a call's three lists with their clamp as k_traffic_count / _scan / _write leave them (the kernels' compaction is
// compact_core.hpp's, which puts entry j of a list at the number of routed entries in front of it).  TEST TOOL.
#define TETRA_HOST_EMUL 1
#include <cstddef>
#include <cstdint>

#include "../../sdrpp-tetra-demodulator_amd/csrc/traffic_core.hpp"

using traffic_core::Slot;

extern "C" {

int traffic_emul_kinds() { return traffic_core::kKinds; }

int traffic_emul_slot_valid(int kind, int usage) { return traffic_core::slot_valid(Slot{ (uint8_t)kind, (uint8_t)usage, { 0, 0 } }) ? 1 : 0; }

// route() per entry: slots [n][4][4 bytes], bbk_bits [n][bits_stride] -> out[n] = the list or -1
void traffic_emul_route(int n, const int32_t* frame_type, const uint32_t* scramb, const uint32_t* time, const uint8_t* slots, const int32_t* bbk_ok,
                        const uint8_t* bbk_bits, int bits_stride, int32_t* out) {
    for (int j = 0; j < n; ++j)
        out[j] = traffic_core::route(frame_type[j], scramb[j], time[j], reinterpret_cast<const Slot*>(slots) + (size_t)j * 4, bbk_ok[j],
                                     bbk_bits + (size_t)j * bits_stride);
}

// A call: entry j is frame any_list[j] of channel any_list[j] / F and BBK row j; table [C][4] -> lists [kinds][max_rows] (untouched past
// the kept rows), counts [kinds][3]
void traffic_emul_lists(int n_any, const int32_t* any_list, int F, const int32_t* frame_type, const uint32_t* scramb, const uint32_t* time,
                        const uint8_t* table, const int32_t* bbk_ok, const uint8_t* bbk_t2, int bbk_stride, int max_rows, int32_t* lists, int32_t* counts) {
    int routed[traffic_core::kKinds] = {};
    for (int j = 0; j < n_any; ++j) {
        const int r = any_list[j];
        const int k = traffic_core::route(frame_type[r], scramb[r], time[r], reinterpret_cast<const Slot*>(table) + (size_t)(r / F) * 4, bbk_ok[j],
                                          bbk_t2 + (size_t)j * bbk_stride);
        if (k < 0) continue;
        if (traffic_core::kept(routed[k], max_rows)) lists[(size_t)k * max_rows + routed[k]] = r;
        routed[k]++;
    }
    for (int k = 0; k < traffic_core::kKinds; ++k) traffic_core::clamp_counts(routed[k], max_rows, counts + traffic_core::kCounts * k);
}

}  // extern "C"
