// resamp_core.hpp -- rational resampler I / DN on time-major frames [frame][channel] (complex64), thread level.
//
// BASELINE config 5 at the plugin's operating point: the channeliser's 800 x 25 kHz channels leave it at 50 ksps (2 x oversampled
// bank); the reference instance is created at VFO_SAMPLERATE 36000 with 2 samples per symbol (/root/reference/src/main.cpp:35,75,84),
// so the frames go through an 18 / 25 polyphase resampler before the demodulator (SURVEY.md section 8(f) #1 names this route).
//
//   y[m][c] = sum_{j < T} h[r_m + I j] x[q_m - j][c],      I q_m + r_m = DN m,  0 <= r_m < I          (include/tetra_chan.h)
//
// = zero-stuff by I, low-pass h (I T taps, gain I), keep every DN-th.  The filter is real and the same for every channel, so a frame
// row is 2 C independent floats: a lane owns a UNIT of W consecutive floats of the row (W = 4: two channels, 16-byte accesses) and one
// GROUP of I consecutive outputs m = I G + i -- a whole turn of the phase wheel, so that r_i = DN i mod I and q_i = floor(DN i / I)
// are compile-time constants of the unrolled loop: the T coefficients of output i are uniform over the wavefront (scalar loads, they
// sit in SGPRs), and of the DN + T - 1 input rows a group reads every one is loaded once and used from registers.  Consecutive lanes
// = consecutive units: every load / store instruction of a wavefront covers one contiguous 1 KB run of a row.
//
// The wideband receiver (tetra_wbrx.hip) runs the same thread code over a channeliser's full rows and keeps only the carriers' bins
// (PickColumns below): every output float is the same fma chain over the same coefficients as the full resampler's, so a picked
// column equals that column of the full resampler bit for bit.
//
// A carrier that lies off its bin's centre is mixed down in the same pass (MixColumns below, include/ext/tetra_carrier_offset.h):
// each row is rotated once, as it is loaded, by a phasor whose phase is formed in integer arithmetic.
//
// Compiles for the host as well (tests/emul/resamp_emul.cpp runs every thread of a launch against the double-precision definition,
// and the picking variant against the full one; tests/emul/resamp_mix_emul.cpp does the same for the mixing variant).
#pragma once

#include <cmath>
#include <cstddef>

#if defined(__HIPCC__) || defined(__HIP__)
#define RESAMP_HD __host__ __device__ __forceinline__
#else
#define RESAMP_HD inline
#endif
#if defined(__clang__)
#define RESAMP_FP_FAST _Pragma("clang fp contract(fast)")
#else
#define RESAMP_FP_FAST
#endif

namespace resamp {

struct alignas(16) f4 { float v[4]; };
struct alignas(8) f2 { float v[2]; };
template <int W> struct unit_of;
template <> struct unit_of<4> { using type = f4; };
template <> struct unit_of<2> { using type = f2; };

struct Ctx {
    const float* x;        // the call's n_in new frames [n_in][2 C] floats, where the caller left them
    const float* hist;     // the T - 1 frames before them, oldest first (the handle's delay line)
    float* out;            // [m1 - m0][2 C]
    const float* coef;     // [I][T]: coef[i][j] = h[r_i + I j], r_i = DN i mod I      (fixed-ratio kernel)
                           // [I T] : the prototype h itself                           (generic kernel)
    long long n0;          // absolute index of the first new frame
    long long m0, m1;      // absolute output indices this call emits: [m0, m1)
    int n_in;
    int units;             // lane units per row: 2 C / W
    int I, DN, T;          // (generic kernel only)
};

// Row `rel` of the stream counted from the call's first new frame.  Interior groups read only new frames (CAREFUL = false).  The
// groups at a call's two ends reach back into the delay line (rel < 0) or ask for rows the call does not hold -- rows that only
// feed outputs outside [m0, m1), which are not stored: those read the nearest row there is.
template <int W, bool CAREFUL> RESAMP_HD typename unit_of<W>::type row_at(const Ctx& c, long long rel, int u, int T) {
    using V = typename unit_of<W>::type;
    const long long stride = (long long)c.units;
    if (!CAREFUL) return reinterpret_cast<const V*>(c.x)[rel * stride + u];
    if (rel < 0) {
        const long long k = (T - 1) + rel;
        return reinterpret_cast<const V*>(c.hist)[(k < 0 ? 0 : k) * stride + u];
    }
    return reinterpret_cast<const V*>(c.x)[(rel < c.n_in ? rel : c.n_in - 1) * stride + u];
}

// Which input column a lane unit reads.  A column map hands each lane a `lane` object whose row() reads the lane's unit of a row.
// A lane may also rotate what it reads: phasor(a0) is what it keeps for a run of rows that starts at absolute frame a0, mixed(v, p, k)
// the row k frames behind a0 as it enters the sums.  AllColumns and PickedLane rotate nothing (NoPhasor: no state, no instruction).
struct NoPhasor {};
// AllColumns (the resampler, tetra_resamp.hip): unit u of rows of c.units units, in the new frames, the delay line and the output.
struct AllColumns {
    RESAMP_HD AllColumns lane(const Ctx&, int) const { return *this; }
    template <int W, bool CAREFUL> RESAMP_HD typename unit_of<W>::type row(const Ctx& c, long long rel, int u, int T) const {
        return row_at<W, CAREFUL>(c, rel, u, T);
    }
    RESAMP_HD NoPhasor phasor(long long) const { return NoPhasor(); }
    template <class V> RESAMP_HD V mixed(const V& v, NoPhasor, int) const { return v; }
};
// PickColumns (the wideband receiver, tetra_wbrx.hip): the new frames are a channeliser's rows of in_units units, of which unit u
// reads column col[u] (one channel per unit: W = 2); the delay line and the output hold the picked columns only (rows of c.units =
// the number of picked columns), unit u.
struct PickedLane {
    long long stride;      // units per row of the new frames
    int col;               // the lane's column in them
    template <int W, bool CAREFUL> RESAMP_HD typename unit_of<W>::type row(const Ctx& c, long long rel, int u, int T) const {
        using V = typename unit_of<W>::type;
        if (!CAREFUL) return reinterpret_cast<const V*>(c.x)[rel * stride + col];
        if (rel < 0) {
            const long long k = (T - 1) + rel;
            return reinterpret_cast<const V*>(c.hist)[(k < 0 ? 0 : k) * (long long)c.units + u];
        }
        return reinterpret_cast<const V*>(c.x)[(rel < c.n_in ? rel : c.n_in - 1) * stride + col];
    }
    RESAMP_HD NoPhasor phasor(long long) const { return NoPhasor(); }
    template <class V> RESAMP_HD V mixed(const V& v, NoPhasor, int) const { return v; }
};
struct PickColumns {
    const int* col;        // [c.units], each in [0, in_units)
    int in_units;
    RESAMP_HD PickedLane lane(const Ctx&, int u) const { return PickedLane{(long long)in_units, col[u]}; }
};

// MixColumns (the wideband receiver's per-carrier offsets, include/ext/tetra_carrier_offset.h): PickColumns whose unit u is rotated by
// exp(-j 2 pi (inc[u] n mod 2^32) / 2^32), n = the row's absolute frame index, before it enters the sums -- the delay line and the
// new frames hold un-rotated rows.  No phase is carried from row to row or from call to call: a run of rows (a group's kRows, a
// generic output's T) takes ONE phasor from the exact integer phase of its first row a0, (inc a0) mod 2^32, and row a0 + k is
// rotated by that phasor times step[k] = exp(-j 2 pi (inc k mod 2^32) / 2^32), a table per slot that the host fills in double when
// the offsets are set (step_table).  The coefficients stay wave-uniform scalars; phasor, steps and products are the lane's own.
struct Phasor { float re, im; };
// exp(-j 2 pi ph / 2^32): the quadrant is taken off in integers (exact), the rest, at most an eighth of a turn either way, goes
// through two short polynomials (Cephes' sinf / cosf kernels; 1.2e-7 at worst with the float32 roundings around them).  ph = 0 gives exactly (1, 0).
RESAMP_HD Phasor phasor_of(unsigned ph) {
    RESAMP_FP_FAST
    const unsigned q = (ph + 0x20000000u) >> 30;
    const int d = (int)(ph - (q << 30));                          // [-2^29, 2^29)
    const float t = (float)d * 1.4629180792671596e-9f;            // 2 pi / 2^32
    const float z = t * t;
    const float s = t + t * z * (-1.6666654611e-1f + z * (8.3321608736e-3f + z * -1.9515295891e-4f));
    const float c = 1.0f - 0.5f * z + z * z * (4.166664568298827e-2f + z * (-1.388731625493765e-3f + z * 2.443315711809948e-5f));
    // (cos, sin) of q quarter turns + t, then the conjugate
    const float co = (q & 1) ? ((q & 2) ? s : -s) : ((q & 2) ? -c : c);
    const float si = (q & 1) ? ((q & 2) ? -c : c) : ((q & 2) ? -s : s);
    return Phasor{co, -si};
}
struct MixedLane {
    PickedLane pick;
    unsigned inc;          // the slot's offset, 2^-32 cycles per frame
    const f2* step;        // the slot's step phasors: step[k * units]
    long long units;
    template <int W, bool CAREFUL> RESAMP_HD typename unit_of<W>::type row(const Ctx& c, long long rel, int u, int T) const {
        return pick.template row<W, CAREFUL>(c, rel, u, T);
    }
    RESAMP_HD Phasor phasor(long long a0) const { return phasor_of(inc * (unsigned)(unsigned long long)a0); }
    RESAMP_HD f2 mixed(const f2& v, const Phasor& p, int k) const {
        RESAMP_FP_FAST
        const f2 s = step[k * units];
        const float re = p.re * s.v[0] - p.im * s.v[1], im = p.re * s.v[1] + p.im * s.v[0];
        f2 o;
        o.v[0] = v.v[0] * re - v.v[1] * im;
        o.v[1] = v.v[0] * im + v.v[1] * re;
        return o;
    }
};
struct MixColumns {
    const int* col;        // [c.units], each in [0, in_units)
    int in_units;
    const unsigned* inc;   // [c.units]
    const f2* step;        // [mix_rows(I, DN, T)][c.units]
    RESAMP_HD MixedLane lane(const Ctx& c, int u) const {
        return MixedLane{PickedLane{(long long)in_units, col[u]}, inc[u], step + u, (long long)c.units};
    }
};

// One group of I outputs (absolute group G, i.e. outputs I G .. I G + I - 1) for lane unit u.
template <int I, int DN, int T, int W, bool CAREFUL, class Lane> RESAMP_HD void group_t(const Ctx& c, long long G, int u, const Lane& lane) {
    RESAMP_FP_FAST
    using V = typename unit_of<W>::type;
    constexpr int kQmax = (DN * (I - 1)) / I;            // newest row the group's last output reads
    constexpr int kRows = kQmax + T;                      // rows -(T - 1) .. kQmax relative to row DN G
    const long long base = (long long)DN * G - c.n0;      // row DN G counted from the call's first new frame
    const auto ph = lane.phasor((long long)DN * G - (T - 1));      // (a mixing lane's; nothing for the others)
    V rows[kRows];
#pragma unroll
    for (int k = 0; k < kRows; k++) rows[k] = lane.mixed(lane.template row<W, CAREFUL>(c, base + (k - (T - 1)), u, T), ph, k);
    V* const out = reinterpret_cast<V*>(c.out);
#pragma unroll
    for (int i = 0; i < I; i++) {
        const int q = (DN * i) / I;                       // compile-time after unrolling
        float acc[W];
#pragma unroll
        for (int w = 0; w < W; w++) acc[w] = 0.f;
#pragma unroll
        for (int j = T - 1; j >= 0; j--) {                 // oldest row first
            const float h = c.coef[i * T + j];
            const V xv = rows[q - j + (T - 1)];
#pragma unroll
            for (int w = 0; w < W; w++) acc[w] += h * xv.v[w];
        }
        const long long m = (long long)I * G + i;
        if (!CAREFUL || (m >= c.m0 && m < c.m1)) {
            V o;
#pragma unroll
            for (int w = 0; w < W; w++) o.v[w] = acc[w];
            out[(m - c.m0) * (long long)c.units + u] = o;
        }
    }
}

// is group G an interior one?  (all I outputs inside [m0, m1) and every row it reads among the new frames)
template <int I, int DN, int T> RESAMP_HD bool group_is_careful(const Ctx& c, long long G) {
    constexpr int kQmax = (DN * (I - 1)) / I;
    const long long base = (long long)DN * G - c.n0;
    return (long long)I * G < c.m0 || (long long)I * G + I > c.m1 || base - (T - 1) < 0 || base + kQmax > (long long)c.n_in - 1;
}

// Thread t of the launch: groups G0 .. of the call x units, flattened (a wavefront may straddle two groups: the coefficients do not
// depend on the group, so they stay wave-uniform).
template <int I, int DN, int T, int W, class Cols = AllColumns> RESAMP_HD void thread_fixed(const Ctx& c, long long t, const Cols& cols = Cols()) {
    const long long G0 = c.m0 / I, G1 = (c.m1 + I - 1) / I;         // groups [G0, G1) hold the call's outputs
    const long long g = t / c.units;
    const int u = (int)(t - g * c.units);
    const long long G = G0 + g;
    if (G >= G1) return;
    const auto lane = cols.lane(c, u);
    if (group_is_careful<I, DN, T>(c, G)) group_t<I, DN, T, W, true>(c, G, u, lane);
    else group_t<I, DN, T, W, false>(c, G, u, lane);
}

// Any ratio, any length (run-time I, DN, T): one output per (thread, unit); coefficients from the prototype in memory.
template <int W, class Cols = AllColumns> RESAMP_HD void thread_generic(const Ctx& c, long long t, const Cols& cols = Cols()) {
    RESAMP_FP_FAST
    using V = typename unit_of<W>::type;
    const long long k = t / c.units;
    const int u = (int)(t - k * c.units);
    const long long m = c.m0 + k;
    if (m >= c.m1) return;
    const long long q = ((long long)c.DN * m) / c.I;
    const int r = (int)((long long)c.DN * m - q * c.I);
    const auto lane = cols.lane(c, u);
    const auto ph = lane.phasor(q - (c.T - 1));
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; w++) acc[w] = 0.f;
    for (int j = c.T - 1; j >= 0; j--) {
        const float h = c.coef[r + c.I * j];
        const V xv = lane.mixed(lane.template row<W, true>(c, q - j - c.n0, u, c.T), ph, c.T - 1 - j);
#pragma unroll
        for (int w = 0; w < W; w++) acc[w] += h * xv.v[w];
    }
    V o;
#pragma unroll
    for (int w = 0; w < W; w++) o.v[w] = acc[w];
    reinterpret_cast<V*>(c.out)[k * (long long)c.units + u] = o;
}

// The ratios and lengths with thread code specialised at compile time (thread_fixed): the one table.  tetra_resamp.hip picks its
// kernels through it and the host emulation its thread code; any other (I, DN, T) runs thread_generic.
template <int I_, int DN_, int T_> struct Ratio { static constexpr int I = I_, DN = DN_, T = T_; };
template <class... R> struct RatioList {};
using Ratios = RatioList<Ratio<18, 25, 8>, Ratio<18, 25, 12>, Ratio<18, 25, 16>, Ratio<18, 25, 24>, Ratio<2, 3, 8>, Ratio<3, 2, 8>, Ratio<1, 2, 8>>;
template <class F, class... R> inline void for_each_ratio(RatioList<R...>, F&& f) { (f(R()), ...); }
// f(Ratio<I, DN, T>()) if the triple is in the table; false ("none") otherwise
template <class F> inline bool visit_ratio(int I, int DN, int T, F&& f) {
    bool found = false;
    for_each_ratio(Ratios(), [&](auto r) {
        if (I == r.I && DN == r.DN && T == r.T) { f(r); found = true; }
    });
    return found;
}

// coef[i][j] = h[(DN i mod I) + I j]
inline void phase_table(const float* h, int I, int DN, int T, float* coef) {
    for (int i = 0; i < I; i++)
        for (int j = 0; j < T; j++) coef[i * T + j] = h[(DN * i) % I + I * j];
}

// The mixing lanes' step phasors.  Rows of the table: the longest run of rows one phasor serves, a group's kRows (>= T, the generic
// kernel's run).  step[k][u] = exp(-j 2 pi (inc[u] k mod 2^32) / 2^32), in double, rounded once.
inline int mix_rows(int I, int DN, int T) { return (int)(((long long)DN * (I - 1)) / I) + T; }
inline void step_table(const unsigned* inc, int units, int rows, float* step) {
    for (int k = 0; k < rows; k++)
        for (int u = 0; u < units; u++) {
            const double th = 6.283185307179586476925286766559 * (double)(unsigned)(inc[u] * (unsigned)k) / 4294967296.0;
            step[2 * ((size_t)k * units + u)] = (float)std::cos(th);
            step[2 * ((size_t)k * units + u) + 1] = (float)-std::sin(th);
        }
}

// outputs that exist once n frames have arrived: m with floor(DN m / I) <= n - 1
inline long long outputs_after(long long n, int I, int DN) { return (n * I + DN - 1) / DN; }

}  // namespace resamp
