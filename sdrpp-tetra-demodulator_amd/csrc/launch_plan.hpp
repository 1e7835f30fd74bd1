// launch_plan.hpp -- which kernel, in which workgroup shapes, a demodulator handle launches: ONE pure function of the channel count,
// the device's CU count, the create flags and the design (host code, plain C++17).  tetra_demod.hip computes the plan wherever a
// design is committed (create, the setters); tetra_demod_process_device only reads it.  Every shape gives the same bits, so no parity
// test sees a wrong plan: tests/test_launch_plan.py holds this against launches recorded on the device (profiles/trace_launch_plan.py).
#pragma once

#include "../../include/tetra_demod.h"
#include "design.hpp"

namespace tdm {
namespace host {

// k_fused's workgroup shapes (kernel_fused.hpp owns them and is device code only: tetra_demod.hip static_asserts these copies)
constexpr int kPlanCh = 16, kPlanChWide = 32, kPlanChSmall = 4;
static_assert(kF4Pad == 68 && kF8Pad == 72, "the 32-channel shape's FLL rows hold 68 taps, the regular rows of the others 72");

constexpr int kWg16ClocksPerSample = 258;       // measured shader clocks per sample of one workgroup round: 3.86 ms per 36000 samples (profiles/r03)
constexpr int kWg32ClocksPerSample = 348;       // 32-channel workgroup: 5.21 ms per 36000 samples
constexpr int kWg4ClocksPerSample = 223;        // 4-channel workgroup: 3.33 ms per 36000 samples

struct LaunchPlan {
    bool generic = false;       // k_generic takes the whole call; nothing below applies
    int n_wide = 0;             // k_fused: channels [0, n_wide) run in 32-channel workgroups ...
    int rest_ch = kPlanCh;      // ... and [n_wide, C) in 16- or 4-channel ones: at most two launches, back to back on the stream
    int deep = 0;               // deep_level() of the design: the symbol ring of the rest's kernel
    bool long_rows = false;     // filters of 73 .. 129 taps: the LONG variant (4- and 16-channel shapes)
};

// Can a launch take the generic kernel (kernel_generic.hpp)?  The design, or TETRA_FLAG_GENERIC_KERNEL, decides.
inline bool generic_applies(int flags, const Design& d) {
    return needs_generic(d) || ((needs_long(d) || deep_level(d) == 2) && (flags & TETRA_FLAG_GENERIC_KERNEL));
}

// k_generic's channels per wave: about eight waves per CU when there are enough channels, never more than 64 channels per wave
inline int generic_lanes(int n_channels, int cus) {
    const int lanes = n_channels / (8 * cus);
    return lanes < 1 ? 1 : lanes > 64 ? 64 : lanes;
}

inline LaunchPlan plan_launch(int n_channels, int cus, int flags, const Design& d) {
    LaunchPlan p;
    // timing loops below 0.07 samples per symbol (with TETRA_FLAG_GENERIC_KERNEL: below 0.27, and filters of more than 72 taps)
    if ((p.generic = generic_applies(flags, d))) return p;
    p.deep = deep_level(d);
    p.long_rows = needs_long(d);
    const bool force_wide = flags & TETRA_FLAG_WIDE_WORKGROUPS, force_narrow = flags & TETRA_FLAG_NARROW_WORKGROUPS, force_small = flags & TETRA_FLAG_SMALL_WORKGROUPS;
    // Workgroup shapes.  16 channels per workgroup is the fastest way through ONE workgroup (kWg16 clocks per sample) and
    // right while there is at most one per CU; the 32-channel workgroup (FLL rows of 4 lanes per channel: the loop code
    // of an FLL wave serves twice the channels; kWg32 clocks per sample) gets a CU through 32 channels in 1.3x that time.
    // Plan: whole rounds of 32-channel workgroups first; what is left takes whichever shape gets it through in less time (rounds of
    // workgroups per CU x clocks per round): one round of 4-channel workgroups (each has a CU to itself and the shortest FLL step:
    // kWg4 clocks per sample) if there are at most 4 channels per CU, else rounds of 16-channel ones, or one more round of 32-channel
    // ones.  The flags force one shape for everything.
    const long long C = n_channels, per_round32 = (long long)kPlanChWide * cus;
    const long long full = (C / per_round32) * per_round32, rest = C - full;
    const long long r16 = ((rest + kPlanCh - 1) / kPlanCh + cus - 1) / cus, r32 = ((rest + kPlanChWide - 1) / kPlanChWide + cus - 1) / cus;
    const long long t16 = r16 * kWg16ClocksPerSample, t32 = r32 * kWg32ClocksPerSample;
    const long long t4 = rest <= (long long)kPlanChSmall * cus ? (long long)kWg4ClocksPerSample : t16 + t32 + 1;
    const bool rest_wide = rest > 0 && t32 < t16 && t32 < t4;
    long long n_wide = force_wide ? C : force_narrow || force_small ? 0 : rest_wide ? C : full;
    const bool small = force_small || (!force_wide && !force_narrow && rest > 0 && !rest_wide && t4 < t16);
    // the 32-channel shape's FLL rows hold 4 x 17 taps and it has neither the deep symbol ring nor long rows: then everything is "the rest"
    if (d.ntaps_be > kF4Pad || p.deep || p.long_rows) n_wide = 0;
    p.n_wide = (int)n_wide;
    // the rest: deep level 2 always takes the 4-channel shape (its 1024-deep ring exists there only); long rows take 4-channel workgroups
    // while every one of them has a CU to itself, 16-channel ones beyond -- or as the flags say
    const bool rest_small = p.deep == 2 || force_small ||
                            (p.long_rows ? !force_wide && !force_narrow && C <= (long long)kPlanChSmall * cus
                                         : small && C - n_wide <= (long long)kPlanChSmall * cus);
    p.rest_ch = rest_small ? kPlanChSmall : kPlanCh;
    return p;
}

}  // namespace host
}  // namespace tdm
