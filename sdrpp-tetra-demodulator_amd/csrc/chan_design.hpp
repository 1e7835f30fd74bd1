// chan_design.hpp -- the window design behind the channeliser's and the resampler's default prototypes (tetra_chan.hip,
// tetra_resamp.hip).  Host-side only, plain C++: tests/emul/chan_design_shim.cpp compiles it on its own and holds it against the
// oracle's restatement (oracle/chan_oracle.c), with which it shares no code.
#pragma once

#include <cmath>
#include <vector>

namespace chandesign {

inline double bessel_i0(double x) {
    double s = 1.0, t = 1.0;
    for (int k = 1; k < 60; k++) {
        t *= (x / (2.0 * k)) * (x / (2.0 * k));
        s += t;
        if (t < 1e-18 * s) break;
    }
    return s;
}

// Kaiser(beta)-windowed sinc of L taps, cutoff fc cycles per sample, DC gain `gain`.
inline void kaiser_sinc(int L, double fc, double beta, double gain, std::vector<float>& out) {
    const double pi = 3.14159265358979323846;
    std::vector<double> t(L);
    double sum = 0.0;
    for (int l = 0; l < L; l++) {
        const double u = (double)l - 0.5 * (double)(L - 1);
        const double sinc = (u == 0.0) ? 2.0 * fc : std::sin(2.0 * pi * fc * u) / (pi * u);
        const double r = L > 1 ? 2.0 * u / (double)(L - 1) : 0.0;
        const double w = bessel_i0(beta * std::sqrt(1.0 - r * r > 0 ? 1.0 - r * r : 0.0)) / bessel_i0(beta);
        t[l] = sinc * w;
        sum += t[l];
    }
    out.resize(L);
    for (int l = 0; l < L; l++) out[l] = (float)(t[l] / sum * gain);
}

}  // namespace chandesign
