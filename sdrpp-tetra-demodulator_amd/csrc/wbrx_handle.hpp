// wbrx_handle.hpp -- the wideband receiver's handle (include/tetra_wbrx.h) as its C ABI sources share it: tetra_wbrx.hip runs the
// stream, tetra_retune.hip retunes its slots (include/tetra_retune.h).  Host-side definitions only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/tetra_shift.h"
#include "hip_host.hpp"
#include "retune_list.hpp"

struct tetra_wbrx {
    tetra_wbrx_config_t cfg;
    int device = 0, last_hip = 0;
    int M = 0, n_bins = 0, max_in = 0, max_chan = 0, max_res = 0;
    bool all = false;                       // bins = 0 .. M - 1 in order: the resampler runs in place on the full rows
    std::vector<int32_t> bins;
    Handle<tetra_chan_t*, tetra_chan_destroy> chan;
    Handle<tetra_resamp_t*, tetra_resamp_destroy> rs;
    Handle<tetra_rx_t*, tetra_rx_destroy> rx;
    DevMem<int32_t> d_bins;                 // [n_bins]
    DevMem<float> chan_out;                 // [max_chan][M] complex64: the latest call's channeliser frames
    DevMem<float> res[2];                   // per call parity: [max_res][n_bins] complex64, the resampled carriers
    int n_res[2] = { 0, 0 };
    int n_chan = 0;                         // channeliser frames of the latest call
    Event ev_chan, ev_res[2], ev_done;
    bool done_recorded = false;             // ev_done has been recorded (by a process call or a retune): later work on any stream waits for it
    long long calls = 0;
    Stream aux;                             // tetra_wbrx_bin_power (created on first use, with its buffers)
    DevMem<double> pw_part;
    DevMem<float> pw_out;
    DevMem<uint8_t> st_x;                   // host-path staging
    // retuning (include/tetra_retune.h, tetra_retune.hip)
    DevMem<float> ring;                     // [T - 1][M] complex64: the channeliser's newest T - 1 frames of ALL bins, frame a in row a mod (T - 1)
    ListRing to_device;                     // a retune's moved slots and their new bins on their way to the device
    long long retunes = 0, slots_changed = 0;
    // per-carrier offsets (include/ext/tetra_carrier_offset.h): the resampler handle holds the list in force and its device tables
    ListRing mix_to_device;                 // a new list's tables on their way to the device
    // stream gaps (include/ext/tetra_gap.h)
    bool at_origin = false;                 // tetra_wbrx_process_device_at has set the stream's origin (forgotten by tetra_wbrx_reset)
    long long at_next = 0;                  // ... and expects this sample index next
};
