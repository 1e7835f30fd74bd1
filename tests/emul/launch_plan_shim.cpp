// launch_plan_shim.cpp -- the product's launch plan (sdrpp-tetra-demodulator_amd/csrc/launch_plan.hpp) behind a C function, for
// tests/test_launch_plan.py (TEST TOOL): the design is rebuilt with host::make_design exactly as tetra_demod_create does.
// Build: g++ -O2 -std=c++17 -shared -fPIC
#include "../../sdrpp-tetra-demodulator_amd/csrc/launch_plan.hpp"

using namespace tdm;

extern "C" {

// out[0..5] = generic, n_wide, rest_ch, deep, long_rows, k_generic's lanes.  Unset parameters: pass a negative value (the config's
// default stays).  Returns 0, or -1 where make_design refuses the parameters.
int launch_plan_shim(int n_channels, int cus, int flags, double samplerate, int rrc_tap_count, int* out) {
    host::DesignParams p;          // tetra_demod_default_config's values (that function lives in the HIP library)
    host::default_timing_gains(p.omega_gain, p.mu_gain);
    if (samplerate >= 0) p.samplerate = samplerate;
    if (rrc_tap_count >= 0) p.rrc_tap_count = rrc_tap_count;
    host::Design d;
    if (!host::make_design(p, nullptr, nullptr, nullptr, d)) return -1;
    const host::LaunchPlan plan = host::plan_launch(n_channels, cus, flags, d);
    out[0] = plan.generic; out[1] = plan.n_wide; out[2] = plan.rest_ch; out[3] = plan.deep; out[4] = plan.long_rows;
    out[5] = host::generic_lanes(n_channels, cus);
    return 0;
}
}
