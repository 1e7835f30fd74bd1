// iqcond_core.hpp -- lane-level code of the capture conditioning (include/ext/tetra_iqcond.h): the per-sample real affine map of (I, Q)
// that the channeliser's loads apply, and the term a sample adds to the capture's statistics.  Host- and device-callable, like the other
// *_core.hpp (tests/emul/iqcond_emul.cpp runs it on the host).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define IQCOND_HD __host__ __device__ __forceinline__
#else
#define IQCOND_HD inline
#endif

namespace iqcond {

// tetra_iq_map_t, field for field (the six floats travel as kernel arguments)
struct Map {
    float m00, m01, m10, m11, c0, c1;
};

// THE contract: two chained fused multiply-adds per component, in this order.  fmaf is a single correctly rounded operation on both
// sides (v_fma_f32 on the device), so host and device agree bit for bit, whatever the contraction mode of the translation unit.
IQCOND_HD void apply(const Map& m, float xr, float xi, float& yr, float& yi) {
    yr = fmaf(m.m01, xi, fmaf(m.m00, xr, m.c0));
    yi = fmaf(m.m11, xi, fmaf(m.m10, xr, m.c1));
}

IQCOND_HD bool finite(const Map& m) {
    return std::isfinite(m.m00) && std::isfinite(m.m01) && std::isfinite(m.m10) && std::isfinite(m.m11) && std::isfinite(m.c0) && std::isfinite(m.c1);
}

// ---- statistics (tetra_iq_stats_device): the five sums of one lane, integer samples exactly, complex64 in double ------------
constexpr int kSums = 5;      // s_i, s_q, s_ii, s_qq, s_iq
template <class T> struct Sums {
    T v[kSums];
};
IQCOND_HD void add_sample(Sums<long long>& s, int i, int q) {      // |i|, |q| <= 2^15: every product fits 32 bits, every sum 64 for n <= 2^32
    s.v[0] += i;
    s.v[1] += q;
    s.v[2] += (long long)i * i;
    s.v[3] += (long long)q * q;
    s.v[4] += (long long)i * q;
}
IQCOND_HD void add_sample(Sums<double>& s, float i, float q) {     // the products of two binary32 values are exact in double
    const double di = (double)i, dq = (double)q;
    s.v[0] += di;
    s.v[1] += dq;
    s.v[2] += di * di;
    s.v[3] += dq * dq;
    s.v[4] += di * dq;
}
template <class T> IQCOND_HD void add_sums(Sums<T>& a, const Sums<T>& b) {
#pragma unroll
    for (int j = 0; j < kSums; j++) a.v[j] += b.v[j];
}

}  // namespace iqcond
