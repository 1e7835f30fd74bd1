// chan_design_shim.cpp -- the product's window design (sdrpp-tetra-demodulator_amd/csrc/chan_design.hpp) behind a C function, for
// tests/test_front_end.py (TEST TOOL): held against the oracle's own restatement of the formula (oracle/chan_oracle.c).
// Build: g++ -O2 -std=c++17 -shared -fPIC
#include <cstring>

#include "../../sdrpp-tetra-demodulator_amd/csrc/chan_design.hpp"

extern "C" {

// out: [L] taps
void chan_design_shim(int L, double fc, double beta, double gain, float* out) {
    std::vector<float> h;
    chandesign::kaiser_sinc(L, fc, beta, gain, h);
    std::memcpy(out, h.data(), sizeof(float) * h.size());
}
}
