// resamp_handle.hpp -- the resampler handle (include/tetra_chan.h, tetra_resamp_*) as its C ABI source and the wideband receiver
// (tetra_wbrx.hip) share it: the receiver owns one and runs it in place or over picked channeliser columns.  Host-side only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/tetra_chan.h"
#include "hip_host.hpp"
#include "resamp_core.hpp"

typedef void (*fixed_kernel_t)(resamp::Ctx, int, long long);
typedef void (*pick_kernel_t)(resamp::Ctx, resamp::PickColumns, int, long long);
typedef void (*mix_kernel_t)(resamp::Ctx, resamp::MixColumns, int, long long);

struct tetra_resamp {
    tetra_resamp_config_t cfg;
    int device = 0, last_hip = 0;
    int C = 0, I = 0, DN = 0, T = 0, W = 4, units = 0, max_in = 0;
    std::vector<float> proto;
    fixed_kernel_t fixed = nullptr;
    pick_kernel_t pick = nullptr;     // the same ratio over picked columns (W = 2; resamp_impl::process_pick_device)
    mix_kernel_t pick_mix = nullptr;  // ... and rotated by the columns' offsets (resamp_impl::set_mix)
    // per-column offsets (include/ext/tetra_carrier_offset.h): empty until the first list that is not all zero
    std::vector<uint32_t> inc;   // [C] the offsets in force, 2^-32 cycles per frame
    bool mixing = false;         // some offset is non-zero: process_pick_device launches the mixing kernels
    DevMem<uint32_t> d_mix;      // [mix_rows][C] complex64 step phasors | [C] offsets (resamp_core.hpp, MixColumns)
    DevMem<float> d_coef;        // [I][T] phase table (fixed kernel) or the prototype (generic)
    DelayLine<float> hist;       // [T - 1][2 C]: the frames before the next call's first
    long long n_total = 0;       // frames consumed so far
    long long m_next = 0;        // outputs emitted so far
    DevMem<float> st_in;         // host-path staging
    DevMem<float> st_out;
    Event ev[2];
    bool ev_valid = false;
};

namespace resamp_impl {

// tetra_resamp_process_device over picked columns: d_in holds [n_in][in_ch] complex64 frames (a channeliser's rows), output column j
// is input column cols[j] resampled, j < the handle's C, bit for bit what the handle would emit for that column on all in_ch.  The
// handle's delay line holds the picked columns.  Needs a handle created with TETRA_RESAMP_FLAG_NARROW_UNITS (W = 2); d_cols: [C]
// device int32, each in [0, in_ch).  Same statuses and stream rules as tetra_resamp_process_device.
__attribute__((visibility("hidden"))) int process_pick_device(tetra_resamp_t* h, const int32_t* d_cols, int in_ch, const float* d_in, int n_in,
                                                            float* d_out, int* n_out, hipStream_t s);

// The per-column offsets of process_pick_device (resamp_core.hpp, MixColumns).  mix_words: 32-bit words of the device tables for C
// columns.  mix_fill: the tables of inc [C] into words [mix_words], the step phasors in double.  set_mix: takes inc [C] as the
// offsets in force; d_tables (device, [mix_words], filled from mix_fill's words) is copied into the handle's own tables on s -- the
// caller orders s behind the last process call and the next one behind s.  d_tables may be null for a list that is all zero: then
// the un-mixed kernels run again and the tables are not read.
__attribute__((visibility("hidden"))) size_t mix_words(const tetra_resamp_t* h);
__attribute__((visibility("hidden"))) void mix_fill(const tetra_resamp_t* h, const uint32_t* inc, int32_t* words);
__attribute__((visibility("hidden"))) int set_mix(tetra_resamp_t* h, const uint32_t* inc, const int32_t* d_tables, hipStream_t s);

}  // namespace resamp_impl
