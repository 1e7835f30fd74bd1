// Host build of the capture conditioning's lane code (csrc/iqcond_core.hpp through chan_fft_core.hpp's conditioned load_sample, the very
// function the kernels' loads call; include/ext/tetra_iqcond.h): sample by sample over a buffer in each of the three formats.  TEST TOOL.
#include <cstdint>

#include "../../sdrpp-tetra-demodulator_amd/csrc/chan_fft_core.hpp"

extern "C" {

// x: n samples in format fmt (0 complex64, 1 cs16, 2 cs8); map: the six coefficients m00, m01, m10, m11, c0, c1; out: [n] complex64
int iqcond_emul_apply(const void* x, int fmt, long long n, const float* map, float* out) {
    const iqcond::Map m = { map[0], map[1], map[2], map[3], map[4], map[5] };
    for (long long s = 0; s < n; s++) {
        chanfft::c32 v;
        if (fmt == chanfft::kFmtC32) v = chanfft::load_sample<chanfft::kFmtC32>(x, s, m);
        else if (fmt == chanfft::kFmtCs16) v = chanfft::load_sample<chanfft::kFmtCs16>(x, s, m);
        else if (fmt == chanfft::kFmtCs8) v = chanfft::load_sample<chanfft::kFmtCs8>(x, s, m);
        else return -1;
        out[2 * s] = v.x;
        out[2 * s + 1] = v.y;
    }
    return 0;
}

int iqcond_emul_map_bytes(void) { return (int)sizeof(iqcond::Map); }

}  // extern "C"
