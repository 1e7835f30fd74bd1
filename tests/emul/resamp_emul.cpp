// resamp_emul.cpp -- host emulation of the rational resampler's kernels, over every column in place and over picked columns (TEST
// TOOL): the product's thread-level source (sdrpp-tetra-demodulator_amd/csrc/resamp_core.hpp: group / unit maps, the interior and the
// careful row accessors of both column maps, the predicated stores, the phase table, the table of specialised ratios) run thread by
// thread over exactly the thread range tetra_resamp.hip launches -- so the index arithmetic is checked against the double-precision
// definition (oracle/chan_oracle.c) without a GPU, and the picking variant bit for bit against the full one followed by a column pick.
// Build: g++ -O2 -std=c++17 -shared -fPIC
#include <cstddef>
#include <vector>

#include "../../sdrpp-tetra-demodulator_amd/csrc/resamp_core.hpp"

using namespace resamp;

namespace {

// Every thread of the call's launch.  cols: none (AllColumns) or one PickColumns, as the kernels of tetra_resamp.hip take them.
// Returns the number of output frames, -1 if (I, DN, T) is not in the product's table and generic == 0.
template <class... Cols> int run(Ctx c, int W, int generic, const float* proto, Cols... cols) {
    const long long n_out = c.m1 - c.m0;
    if (n_out == 0) return 0;
    constexpr int kThreads = 256;
    if (generic) {
        c.coef = proto;
        const long long blocks = (n_out * c.units + kThreads - 1) / kThreads;
        for (long long t = 0; t < blocks * kThreads; t++) {
            if (W == 4) thread_generic<4>(c, t, cols...);
            else thread_generic<2>(c, t, cols...);
        }
        return (int)n_out;
    }
    std::vector<float> coef((size_t)c.I * c.T);
    phase_table(proto, c.I, c.DN, c.T, coef.data());
    c.coef = coef.data();
    const long long threads0 = ((c.m1 + c.I - 1) / c.I - c.m0 / c.I) * (long long)c.units;
    const long long threads = (threads0 + kThreads - 1) / kThreads * kThreads;
    const bool found = visit_ratio(c.I, c.DN, c.T, [&](auto r) {
        using R = decltype(r);
        for (long long t = 0; t < threads; t++) {
            if (W == 4) thread_fixed<R::I, R::DN, R::T, 4>(c, t, cols...);
            else thread_fixed<R::I, R::DN, R::T, 2>(c, t, cols...);
        }
    });
    return found ? (int)n_out : -1;
}

}  // namespace

extern "C" {

// cols == NULL: hist [T - 1][C] complex before the call; x [n_in][C]; out [m1 - m0][C]; lane units of W floats.
// cols != NULL: x [n_in][in_ch] (full channeliser rows), of which output column j is input column cols[j], j < C; hist and out hold
// the C picked columns; W must be 2, as tetra_resamp.hip asks.  proto: [I T].  generic != 0: the run-time-ratio kernel.
int resamp_emul(int I, int DN, int T, int C, int W, int generic, const float* proto, const float* hist, const float* x, int n_in,
                long long n_total, long long m_next, float* out, int in_ch, const int* cols) {
    Ctx c;
    c.x = x; c.hist = hist; c.out = out;
    c.n0 = n_total; c.m0 = m_next; c.m1 = outputs_after(n_total + n_in, I, DN); c.n_in = n_in; c.units = 2 * C / W;
    c.I = I; c.DN = DN; c.T = T;
    if (!cols) return run(c, W, generic, proto);
    if (W != 2) return -1;
    PickColumns pc;
    pc.col = cols; pc.in_units = in_ch;
    return run(c, W, generic, proto, pc);
}

// the product's table of specialised ratios: up to cap triples (I, DN, T) into out; returns how many there are
int resamp_emul_ratios(int* out, int cap) {
    int n = 0;
    for_each_ratio(Ratios(), [&](auto r) {
        if (n < cap) { out[3 * n] = r.I; out[3 * n + 1] = r.DN; out[3 * n + 2] = r.T; }
        n++;
    });
    return n;
}
}
