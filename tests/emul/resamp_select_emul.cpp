// resamp_select_emul.cpp -- host emulation of the wideband receiver's selecting resampler (TEST TOOL): the product's thread-level
// source (sdrpp-tetra-demodulator_amd/csrc/resamp_core.hpp with the PickColumns map) run thread by thread over exactly the thread
// range tetra_resamp.hip launches for picked columns, so that it can be held bit for bit against the full resampler's host build
// (resamp_emul.cpp) followed by a column pick.
// Build: g++ -O2 -std=c++17 -shared -fPIC
#include <cstddef>
#include <vector>

#include "../../sdrpp-tetra-demodulator_amd/csrc/resamp_core.hpp"

using namespace resamp;

namespace {
template <int I, int DN, int T> void run_fixed(const Ctx& c, const PickColumns& cols, long long threads) {
    for (long long t = 0; t < threads; t++) thread_fixed<I, DN, T, 2>(c, t, cols);
}
}  // namespace

extern "C" {

// hist: [T - 1][n_cols] complex (the picked delay line); x: [n_in][in_ch] (full channeliser rows); cols: [n_cols]; out: [m1 - m0][n_cols].
// Returns the number of output frames, -1 if the (I, DN, T) has no specialised kernel and generic == 0.
int resamp_select_emul(int I, int DN, int T, int in_ch, int n_cols, const int* cols, int generic, const float* proto, const float* hist,
                       const float* x, int n_in, long long n_total, long long m_next, float* out) {
    const long long m1 = outputs_after(n_total + n_in, I, DN);
    Ctx c;
    c.x = x; c.hist = hist; c.out = out;
    c.n0 = n_total; c.m0 = m_next; c.m1 = m1; c.n_in = n_in; c.units = n_cols;
    c.I = I; c.DN = DN; c.T = T;
    PickColumns pc;
    pc.col = cols; pc.in_units = in_ch;
    if (m1 == m_next) return 0;
    constexpr int kThreads = 256;
    if (generic) {
        c.coef = proto;
        const long long blocks = ((m1 - m_next) * c.units + kThreads - 1) / kThreads;
        for (long long t = 0; t < blocks * kThreads; t++) thread_generic<2>(c, t, pc);
        return (int)(m1 - m_next);
    }
    std::vector<float> coef((size_t)I * T);
    phase_table(proto, I, DN, T, coef.data());
    c.coef = coef.data();
    const long long threads0 = ((m1 + I - 1) / I - m_next / I) * (long long)c.units;
    const long long threads = (threads0 + kThreads - 1) / kThreads * kThreads;
    if (I == 18 && DN == 25 && T == 16) run_fixed<18, 25, 16>(c, pc, threads);
    else if (I == 18 && DN == 25 && T == 8) run_fixed<18, 25, 8>(c, pc, threads);
    else if (I == 2 && DN == 3 && T == 8) run_fixed<2, 3, 8>(c, pc, threads);
    else return -1;
    return (int)(m1 - m_next);
}
}
