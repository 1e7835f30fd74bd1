// chan_emul.cpp -- host emulation of the channeliser's FFT kernel, un-shifted and frequency-shifted (TEST TOOL): the product's
// lane-level source (sdrpp-tetra-demodulator_amd/csrc/chan_fft_core.hpp: fold with real or complex taps, 32-point FFT, 5 x 5 DFT, the
// frame phasor written by one thread per frame and the store that applies it, LDS layouts, thread -> slot / lane maps) run thread by
// thread, phase by phase, exactly as k_channelise_fft<P, 0, FMT, SHIFT> arranges them between its barriers -- so the index maps,
// the transforms, the shifted arithmetic, the integer phases and the phasor's LDS slot are checked against the double-precision
// definition (oracle/chan_oracle.c) without a GPU.  (The shifted taps and the phasor go through the host's double sin / cos here, the
// phasor through sincospif on the device: both within an ulp of the exact value, so host and device agree to a tolerance there,
// not bit for bit.  The un-shifted path calls no libm function.)
// Build: g++ -O2 -std=c++17 -shared -fPIC
#include <cmath>
#include <type_traits>
#include <vector>

#include "../../sdrpp-tetra-demodulator_amd/csrc/chan_fft_core.hpp"

using namespace chanfft;

namespace {

template <int PP, bool SHIFT> void run(BlockCtx c, int fmt, const float* h, uint32_t inc, int blocks) {
    // the taps as tetra_chan_create / tetra_chan_set_shift lay them out for the fold
    std::vector<float> ht((size_t)(SHIFT ? 4 : 2) * kM * PP);
    if (SHIFT) fold_transpose_prototype(PP, [&](int l) { return modulated_tap(h, inc, l); }, reinterpret_cast<c32*>(ht.data()));
    else fold_transpose_prototype(PP, [&](int l) { return h[l]; }, ht.data());
    c.h = ht.data();
    c.inc = inc;
    std::vector<c32> lds((size_t)kBlockFrames * kFrameLds);
    struct Regs { c32 x[32]; };
    std::vector<Regs> regs(256);
    std::vector<char> live(256);
    for (int blk = 0; blk < blocks; blk++) {
        // the whole block's LDS is poisoned first, pads included: the phasor slot must have been written by phase_phasor, and by
        // nothing else, when the store reads it
        for (auto& v : lds) v = mk(NAN, NAN);
        for (int tid = 0; tid < 256; tid++) {
            if (fmt == kFmtCs16) phase_fold<PP, kFmtCs16, SHIFT>(c, blk, tid, lds.data());
            else if (fmt == kFmtCs8) phase_fold<PP, kFmtCs8, SHIFT>(c, blk, tid, lds.data());
            else phase_fold<PP, kFmtC32, SHIFT>(c, blk, tid, lds.data());
            if (SHIFT) phase_phasor(c, blk, tid, lds.data());
        }
        for (int tid = 0; tid < 256; tid++) live[tid] = phase_fft32_compute(tid, lds.data(), regs[tid].x);      // every lane reads ...
        for (int tid = 0; tid < 256; tid++) if (live[tid]) phase_fft32_store(tid, lds.data(), regs[tid].x);       // ... before any lane writes
        for (int tid = 0; tid < 256; tid++) {
            c32 tw[kN1 - 1];
            load_twiddles(c, tid, tw);
            phase_dft25_store<0, SHIFT>(c, (long long)kBlockFrames * blk, tid, lds.data(), tw);
        }
    }
}

}  // namespace

extern "C" {

// hist: the L - 1 samples before the call (oldest first, always complex64); x: the call's n_in new samples in format fmt (kFmtC32 /
// kFmtCs16 / kFmtCs8: interleaved float / int16 / int8 I, Q pairs) -- two separate buffers, like the kernel sees them; out:
// [frames][800] complex.  P in {4, 6, 8}.  inc: the frequency shift (2^-32 cycles per sample).  mode 0: the library's dispatch -- inc
// == 0 runs the un-shifted instantiations; mode 1: the shifted instantiations whatever inc is (inc == 0: taps (h, 0), phasor 1).
// Returns frames.
int chan_fft_emul(const float* hist, const void* x, int fmt, int n_in, int P, int ph0, long long abs0, const float* h, unsigned inc, int mode,
                  float* out) {
    const int L = kM * P, D = kM / 2;
    const int frames = (ph0 + n_in) / D;
    std::vector<c32> tw((size_t)kN1 * kN2);
    const double pi = 3.14159265358979323846;
    for (int n1 = 0; n1 < kN1; n1++)
        for (int k2 = 0; k2 < kN2; k2++) {
            const double a = -2.0 * pi * (double)((n1 * k2) % kM) / kM;
            tw[(size_t)n1 * kN2 + k2] = mk((float)std::cos(a), (float)std::sin(a));
        }
    BlockCtx c;
    c.x = x;
    c.hist = reinterpret_cast<const c32*>(hist);
    c.n_in = n_in;
    c.out = reinterpret_cast<c32*>(out);
    c.h = nullptr; c.tw = tw.data(); c.frames = frames; c.ph0 = ph0; c.abs0 = abs0; c.L = L; c.inc = 0;
    const int blocks = (frames + kBlockFrames - 1) / kBlockFrames;
    const bool shift = mode == 1 || inc != 0;
    auto go = [&](auto Ptag) {
        constexpr int PP = decltype(Ptag)::value;
        if (shift) run<PP, true>(c, fmt, h, inc, blocks);
        else run<PP, false>(c, fmt, h, inc, blocks);
    };
    if (P == 8) go(std::integral_constant<int, 8>());
    else if (P == 6) go(std::integral_constant<int, 6>());
    else if (P == 4) go(std::integral_constant<int, 4>());
    else return -1;
    return frames;
}

// exp(-j 2 pi ph / 2^32) as the kernels' one thread per frame evaluates it (host branch of shift_phasor)
void chan_shift_phasor(unsigned ph, float* out) {
    const c32 w = shift_phasor(ph);
    out[0] = w.x;
    out[1] = w.y;
}

// The taps of a shifted handle in both layouts tetra_chan_set_shift builds: lin [L] complex (the matrix and direct kernels), fold
// [800][2][P] complex (the FFT kernel).
void chan_shift_taps(const float* h, int P, unsigned inc, float* lin, float* fold) {
    auto tap = [&](int l) { return modulated_tap(h, inc, l); };
    for (int l = 0; l < kM * P; l++) reinterpret_cast<c32*>(lin)[l] = tap(l);
    fold_transpose_prototype(P, tap, reinterpret_cast<c32*>(fold));
}

// the two register-level transforms on their own (natural order in and out)
void chan_fft32(const float* in, float* out) {
    c32 x[32];
    for (int i = 0; i < 32; i++) x[i] = mk(in[2 * i], in[2 * i + 1]);
    fft32_dif(x);
    for (int p = 0; p < 32; p++) { out[2 * bitrev5(p)] = x[p].x; out[2 * bitrev5(p) + 1] = x[p].y; }
}
void chan_dft25(const float* in, float* out) {
    c32 x[25];
    for (int i = 0; i < 25; i++) x[i] = mk(in[2 * i], in[2 * i + 1]);
    dft25(x);
    for (int i = 0; i < 25; i++) { out[2 * i] = x[i].x; out[2 * i + 1] = x[i].y; }
}
}
