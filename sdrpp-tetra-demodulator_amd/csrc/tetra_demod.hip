// tetra_demod.hip -- HIP kernels (gfx950) + C ABI of the batched TETRA pi/4-DQPSK demodulator.
//
// The whole chain runs in ONE kernel, k_fused (kernel_fused.hpp): AGC -> band-edge FLL -> RRC matched filter -> ML timing
// recovery -> pi/4 Costas -> slicer -> differential decoder -> bit unpacker, as specialised waves connected by LDS rings.  Three
// workgroup shapes of the one template: 16 channels in six waves (one workgroup per CU up to 4096 channels), 32 channels in
// eight waves (more than 16 channels per CU) and 4 channels (at most 4 channels per CU); host::plan_launch (launch_plan.hpp) says
// which channels take which shape -- computed wherever a design is committed (create, the setters), read by every process call --
// and the results are identical bit for bit.  Filters of 73 .. 129 taps take the LONG variant of the 4- or
// the 16-channel shape (FLL rows of 16 x 9 / 8 x 17 taps, 128 delay-line samples); timing loops below 0.07 samples per symbol -- and, on request, the
// long filters -- run in k_generic (kernel_generic.hpp): one lane per channel, same arithmetic.  (The two-kernel pipeline of
// round 1 -- k1_agc_fll_rrc / k2_sync_slice with an HBM scratch in between -- was retired in ABI 2; `git log` has it.)
// Reference path replaced: src/dsp/pi4dqpsk.cpp:132-140, src/dsp/dqpsk_sym_extr.cpp:4-55,
// src/dsp/bit_unpacker.cpp:4-10 (see include/tetra_demod.h).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/tetra_demod.h"
#include "constellation_core.hpp"
#include "demod_core.hpp"
#include "design.hpp"
#include "hip_host.hpp"
#include "launch_plan.hpp"
#include "retune_impl.hpp"

using namespace tdm;

namespace {

constexpr int kTinyCallSamples = 768;           // tetra_demod_process: calls of at most this many samples per channel run in place (below)
constexpr int kYHist = kInterpTaps - 1;         // COMPLEX_FD's delay buffer: 7 RRC outputs in front of the new ones

__device__ __forceinline__ Pair<float> ld_pair(const float2* p) {
    float2 v = *p;
    return Pair<float>(v.x, v.y);
}

}  // namespace

#include "kernel_fused.hpp"
#include "kernel_generic.hpp"

namespace {

// Device self-test of the primitives the arithmetic contract rests on (DPP row moves, sqrt, sincos).
// out[0][l] = row_shr1(old = 100+l, src = l), out[1][l] = row_shl1(old = 200+l, src = l),
// out[2][l] = sqrt(in[l]), out[3][l] / out[4][l] = sin / cos of in[64 + l].
__global__ void k_selftest(const float* in, float* out) {
    const int l = threadIdx.x;
    out[l] = row_shr1(100.0f + (float)l, (float)l);
    out[64 + l] = row_shl1(200.0f + (float)l, (float)l);
    out[128 + l] = v_sqrt(in[l]);
    float s, c;
    sincos_t<float>(in[64 + l], s, c);
    out[192 + l] = s;
    out[256 + l] = c;
}

// Matrix-pipe self-test: D = A . B accumulated over K in ASCENDING k by chained
// v_mfma_f32_16x16x4_f32 (M = N = 16) or v_mfma_f32_32x32x2_f32 (M = N = 32) from C = +0 -- to be compared on the host with
// the oracle's fmaf chain `for k: acc = fmaf(A[i][k], B[k][j], acc)`, bit for bit (incl. zero taps, -0, subnormals).
// A [M][K] row-major, B [K][N] row-major, D [M][N] row-major; K a multiple of 4; one wave.
typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));
typedef float mfma_f32x16 __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(64) void k_mfma_selftest(int shape, int K, const float* __restrict__ A, const float* __restrict__ B,
                                                      float* __restrict__ D) {
    const int l = threadIdx.x;
    if (shape == 16) {
        mfma_f32x4 acc = { 0.f, 0.f, 0.f, 0.f };
        for (int kb = 0; kb < K; kb += 4) {
            const float a = A[(l & 15) * K + kb + (l >> 4)];
            const float b = B[(kb + (l >> 4)) * 16 + (l & 15)];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        for (int r = 0; r < 4; r++) D[((l >> 4) * 4 + r) * 16 + (l & 15)] = acc[r];
    } else {
        mfma_f32x16 acc;
        for (int r = 0; r < 16; r++) acc[r] = 0.f;
        for (int kb = 0; kb < K; kb += 2) {
            const float a = A[(l & 31) * K + kb + (l >> 5)];
            const float b = B[(kb + (l >> 5)) * 32 + (l & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        for (int r = 0; r < 16; r++) D[((r & 3) + 8 * (r >> 2) + 4 * (l >> 5)) * 32 + (l & 31)] = acc[r];
    }
}

// Small helper kernels for state management.
__global__ void k_fill_f32(float* p, float v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void k_fill_i32(int* p, int v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
// Host-path helpers (tetra_demod_process_async).
// int16 IQ as most SDR hardware delivers it -> the complex float the chain computes on; x / 32768 is exact in binary32.
__global__ void k_cs16_to_cf32(const short2* __restrict__ in, float2* __restrict__ out, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const short2 v = in[i];
        out[i] = make_float2((float)v.x * (1.0f / 32768.0f), (float)v.y * (1.0f / 32768.0f));
    }
}
// int8 IQ (RTL-SDR / HackRF class front-ends): x / 128, exact.
__global__ void k_cs8_to_cf32(const char2* __restrict__ in, float2* __restrict__ out, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const char2 v = in[i];
        out[i] = make_float2((float)v.x * (1.0f / 128.0f), (float)v.y * (1.0f / 128.0f));
    }
}
// One time chunk's bits appended to the call's output rows: out[c][out_n[c] ..] = chunk[c][0 .. chunk_n[c]).
__global__ void k_append_bits(const uint8_t* __restrict__ chunk, int chunk_stride, const int* __restrict__ chunk_n,
                              uint8_t* __restrict__ out, int out_stride, int* __restrict__ out_n) {
    const int c = blockIdx.x;
    const int at = out_n[c];
    int n = chunk_n[c];
    n = at + n > out_stride ? out_stride - at : n;
    const uint8_t* src = chunk + (size_t)c * chunk_stride;
    uint8_t* dst = out + (size_t)c * out_stride + at;
    for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    if (threadIdx.x == 0) out_n[c] = at + n;
}
// TETRA_FLAG_QUALITY: DQPSKSymbolExtractor's statistic (dqpsk_sym_extr.cpp:8-31) brought up to date after a launch, one
// 64-lane workgroup per channel.  The reference pushes one angular distance per symbol into a 4096-entry ring and, every 256
// symbols, publishes the ring's mean -- summed in float, in ring-index order (:19-23).  Only the value at the LAST such
// boundary of a call can be observed, so the workgroup rebuilds the ring as it stood at that boundary in LDS (old entries,
// overwritten by this call's distances up to the boundary), one lane adds it up in exactly the reference's order, then the
// image and the few symbols behind the boundary go to the ring in memory and the two counters advance.
__global__ __launch_bounds__(64) void k_quality(const float2* __restrict__ sym, long long sym_stride, const int* __restrict__ n_bits,
                                                float* __restrict__ ring, int* __restrict__ q_ptr, int* __restrict__ q_disp,
                                                float* __restrict__ q_err, int* __restrict__ q_sync) {
    __shared__ __attribute__((aligned(16))) float img[4096];
    const int c = blockIdx.x, lane = threadIdx.x;
    const float2* z = sym + (long long)c * sym_stride;
    float* r = ring + (long long)c * 4096;
    const int n = n_bits[c] / 2, ptr0 = q_ptr[c], disp0 = q_disp[c];
    const int total = disp0 + n;
    const int b = total >= 256 ? n - (total & 255) : 0;     // symbols of this call consumed at the last boundary (0 = none)
    if (b > 0) {
        if (b < 4096)                                       // entries this call has not reached by then keep their old value
            for (int i = lane; i < 4096; i += 64) img[i] = r[i];
        __syncthreads();
        for (int j = (b > 4096 ? b - 4096 : 0) + lane; j < b; j += 64) img[(ptr0 + j) & 4095] = tdm::quality_distance(z[j].x, z[j].y);
        __syncthreads();
        if (lane == 0) {
            float xerr = 0.0f;                              // dqpsk_sym_extr.cpp:20-23: float accumulator, index order
            const float4* q = reinterpret_cast<const float4*>(img);
            for (int i0 = 0; i0 < 1024; i0 += 16) {        // sixteen LDS loads in flight, then their 64 adds in order
                float4 v[16];
                _Pragma("unroll")
                for (int k = 0; k < 16; k++) v[k] = q[i0 + k];
                _Pragma("unroll")
                for (int k = 0; k < 16; k++) { xerr += v[k].x; xerr += v[k].y; xerr += v[k].z; xerr += v[k].w; }
            }
            xerr = xerr / 4096.0f;
            q_err[c] = xerr;
            q_sync[c] = xerr >= 0.35f ? 0 : 1;
        }
        for (int i = lane; i < 4096; i += 64) r[i] = img[i];        // the ring at the boundary ...
        __syncthreads();
    }
    // ... and the (fewer than 256) symbols behind it
    for (int j = b + lane; j < n; j += 64) r[(ptr0 + j) & 4095] = tdm::quality_distance(z[j].x, z[j].y);
    if (lane == 0) {
        q_ptr[c] = (ptr0 + n) & 4095;
        q_disp[c] = total & 255;
    }
}

// TETRA_FLAG_CONSTELLATION: the plugin's constellation tap (src/main.cpp:85-89: Reshaper keep 1024 / skip 0 -> :376-383 copies each
// 1024-symbol block to the diagram) brought up to date after a launch, one workgroup per channel (constellation_core.hpp).
constexpr int kCdSyms = tetra_cd::kSyms;
static_assert(kCdSyms == TETRA_CONSTELLATION_SYMBOLS, "header and kernel agree on the block length");
__global__ __launch_bounds__(256) void k_constellation(const float2* __restrict__ sym, long long sym_stride, const int* __restrict__ n_bits,
                                                       float2* __restrict__ blk, float2* __restrict__ part, int* __restrict__ fill,
                                                       int* __restrict__ blocks) {
    const int c = blockIdx.x, tid = threadIdx.x;
    const float2* z = sym + (long long)c * sym_stride;
    float2* B = blk + (long long)c * kCdSyms;
    float2* P = part + (long long)c * kCdSyms;
    const int n = n_bits[c] / 2, f0 = fill[c];
    const tetra_cd::Plan p = tetra_cd::plan(f0, n);
    tetra_cd::assemble_block(p, tid, 256, z, P, B);
    __syncthreads();
    tetra_cd::carry_partial(p, f0, n, tid, 256, z, P);
    if (tid == 0) { fill[c] = p.r; blocks[c] += p.nb; }
}

__global__ void k_min_i32(int* p, int v, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && p[i] > v) p[i] = v;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Host side: handle + C ABI
// ------------------------------------------------------------------------------------------------
struct tetra_demod {
    tetra_demod_config_t cfg;
    host::DesignParams dp;
    host::Design design;
    int device = 0;
    int last_hip = 0;
    int C = 0;
    int max_samples = 0;
    // device memory
    DevMem<float> agc_g, fll_ph, fll_fr;
    DevMem<float2> hist;
    DevMem<float2> hist_far;        // [C][48]: the delay-line samples before hist's 80 (the fused kernel's long rows and the generic kernel)
    bool far_valid = true;          // false once the fused kernel has run since hist_far was written: it then reads as zeros
    DevMem<float2> g_xs, g_ys;      // generic kernel's scratch: [C][128 + max_samples] FLL outputs, [C][7 + max_samples] RRC outputs
    DevMem<float> d_g_be_a, d_g_be_b, d_g_rrc;   // un-padded tap tables for it, [kGenMaxTaps] each
    DevMem<float> mu, omega, cph, cfr, ph2;
    DevMem<int> offset, prev;
    int cus = 256;
    host::LaunchPlan plan;      // what a process call launches under `design` (launch_plan.hpp): set wherever a design is committed
    DevMem<int> rrc_valid;      // [C] delay-line samples the RRC may see (tetra_demod.h: tetra_demod_channel_state.rrc_valid)
    DevMem<float2> y;           // TETRA_FLAG_KEEP_RRC_OUT: time-major RRC output scratch [(7 + max_samples)][C]
    DevMem<float2> ybuf;        // COMPLEX_FD delay buffer [C][7]
    DevMem<int> d_overruns;     // [1] channels cut off at their row capacity, counted by the kernels since create
    long long overruns_seen = 0;   // ... and what the host entry points have already reported of it
    int* cut_flag = nullptr;    // set around an in-place call's launch: a cut-off channel also stores 1 here (mapped host memory)
    bool tn_disabled = false;   // the platform refused the mapped, coherent host blocks: short calls keep the copy-engine path
    DevMem<float> q_ring;       // TETRA_FLAG_QUALITY: [C][4096] distance ring + per-channel state (k_quality)
    DevMem<int> q_ptr, q_disp, q_sync;
    DevMem<float> q_err;
    DevMem<float2> q_sym;       // [C][q_sym_stride] symbols of the last launch when the caller did not ask for them
    DevMem<float2> cd_blk, cd_part;   // TETRA_FLAG_CONSTELLATION: [C][1024] last complete / partial block (k_constellation)
    DevMem<int> cd_fill, cd_blocks;   // [C] symbols in the partial block, blocks completed
    bool taps_sym() const { return q_ring || cd_blk; }      // a post-launch kernel reads the launch's symbols
    long long q_sym_stride = 0;
    bool user_rrc = false, user_be = false;   // caller-supplied FIR tables (cfg.rrc_taps / cfg.bandedge_taps)
    bool quirks = false;        // TETRA_FLAG_REFERENCE_QUIRKS
    bool keep_y = false;        // y scratch allocated
    DevMem<float> d_bank;
    DevMem<float> d_be_re80, d_be_im80, d_rrc_ext;   // band-edge taps zero-padded (old end) to 80, RRC zero-extended
    // host-path staging
    DevMem<float> st_iq;
    DevMem<uint8_t> st_bits;
    DevMem<int> st_nbits;
    DevMem<float> st_sym;
    // small synchronous calls (the single-channel drop-in's 180-sample chunks): page-locked host staging, one packed output
    DevMem<uint8_t> pk_dev;
    HostMem<uint8_t> pk_host, pk_in;
    // the smallest synchronous calls: page-locked, mapped, coherent blocks the kernels read / write in place (no copy engine)
    HostMem<uint8_t> tn_out, tn_in;
    uint8_t *tn_out_dev = nullptr, *tn_in_dev = nullptr;
    // ring of HIP-event pairs (before / after the call's launches), one slot per process call
    static constexpr int kEvSlots = 64;
    Event ev[kEvSlots][2];
    long long n_calls = 0;      // process calls that launched kernels
    Stream own_stream;          // tetra_demod_process_resident: the handle's own (non-blocking) stream
    DevMem<long long> d_prof;   // TETRA_DEMOD_PROFILE scratch
    int last_n = 0;
    // tetra_demod_process_async: three streams, time chunks double-buffered in HBM (see the function)
    struct Async {
        bool ready = false;
        Stream s_in, s_k, s_out;
        Event ev_in[2], ev_free[2], ev_done[2], ev_out[2];
        DevMem<void> d_raw[2];      // int16 input only: the chunk as it came
        DevMem<float> d_iq[2];      // the chunk as complex float [C][chunk] (or [chunk][C])
        DevMem<uint8_t> d_cbits[2]; // the chunk's bits [C][chunk_stride]
        DevMem<int> d_cnb[2];
        DevMem<uint8_t> d_out[2];   // a call's bits [C][bits_stride]; two calls may be in flight
        DevMem<int> d_onb[2];
        long long chunks = 0, calls = 0;
    } as;
};

namespace {

int upload_tables(tetra_demod* h) {
    HIP_TRY(h, hipMemcpy(h->d_bank, h->design.bank.data(), sizeof(float) * kInterpPhases * kInterpTaps,
                         hipMemcpyHostToDevice));
    {   // the generic kernel's un-padded tables (any accepted tap count)
        std::vector<float> a(kGenMaxTaps, 0.f), b(kGenMaxTaps, 0.f), r(kGenMaxTaps, 0.f);
        for (int k = 0; k < h->design.ntaps_be; k++) { a[k] = h->design.be_re[k]; b[k] = h->design.be_im[k]; }
        for (int k = 0; k < h->design.ntaps; k++) r[k] = h->design.rrc[k];
        HIP_TRY(h, hipMemcpy(h->d_g_be_a, a.data(), sizeof(float) * kGenMaxTaps, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_g_be_b, b.data(), sizeof(float) * kGenMaxTaps, hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(h->d_g_rrc, r.data(), sizeof(float) * kGenMaxTaps, hipMemcpyHostToDevice));
    }
    // the fused kernel's padded tables; filters of 73 .. 129 taps: the same tables in the long rows' sizes (kernel_fused.hpp: LONG)
    const bool long_tables = h->design.ntaps > kF8Pad || h->design.ntaps_be > kF8Pad;
    const int be_pad = long_tables ? kBePadLong : kBePad, rrc_ext = long_tables ? kRrcExtLong : kRrcExt;
    std::vector<float> re(be_pad, 0.f), im(be_pad, 0.f), rrx(rrc_ext, 0.f);
    const int o = be_pad - h->design.ntaps_be;
    const int rpad = (8 - ((h->design.ntaps - 1) & 7)) & 7;     // RRC windows start on a multiple of 8, see kernel_fused.hpp
    for (int k = 0; k < h->design.ntaps_be; k++) {
        re[o + k] = h->design.be_re[k];
        im[o + k] = h->design.be_im[k];
    }
    for (int k = 0; k < h->design.ntaps; k++) rrx[7 + rpad + k] = h->design.rrc[k];
    HIP_TRY(h, hipMemcpy(h->d_be_re80, re.data(), sizeof(float) * be_pad, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_be_im80, im.data(), sizeof(float) * be_pad, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->d_rrc_ext, rrx.data(), sizeof(float) * rrc_ext, hipMemcpyHostToDevice));
    return TETRA_OK;
}

int fill(tetra_demod* h, float* p, float v, int first, int count) {
    if (count <= 0) return TETRA_OK;
    hipLaunchKernelGGL(k_fill_f32, dim3((count + 255) / 256), dim3(256), 0, 0, p + first, v, count);
    HIP_TRY(h, hipGetLastError());
    return TETRA_OK;
}

// reset of the timing-recovery loop only (COMPLEX_FD::reset / setOmega, complex_fd.cpp:30-41,78-87)
int reset_timing(tetra_demod* h, int first, int count) {
    int rc;
    if ((rc = fill(h, h->mu, 0.0f, first, count))) return rc;
    if ((rc = fill(h, h->omega, h->design.tr_omega, first, count))) return rc;
    HIP_TRY(h, hipMemsetAsync(h->offset + first, 0, sizeof(int) * count, 0));
    return TETRA_OK;
}

// PI4DQPSK::reset (pi4dqpsk.cpp:120-130) for channels [first, first+count); `fresh` = also everything the reference's
// reset leaves alone (a new handle, and every reset without TETRA_FLAG_REFERENCE_QUIRKS).
int reset_range(tetra_demod* h, int first, int count, bool fresh) {
    int rc;
    // FastAGC::reset -> initGain 1.0; FLL::reset fll.cpp:120-127; FIR::reset clears the delay line (ONE delay line for the
    // three FIRs here, see tetra_demod.h); PLL::reset; COMPLEX_FD::reset complex_fd.cpp:78-87
    if ((rc = fill(h, h->agc_g, 1.0f, first, count))) return rc;
    HIP_TRY(h, hipMemsetAsync(h->fll_ph + first, 0, sizeof(float) * count, 0));
    HIP_TRY(h, hipMemsetAsync(h->fll_fr + first, 0, sizeof(float) * count, 0));
    // FIR::reset: the reference clears the RRC's delay line only; FLL::reset leaves the band-edge FIRs' lines alone.  To the
    // letter (quirks, fused pipeline) the shared line therefore stays and the RRC is told to see none of it.
    if (fresh) {
        HIP_TRY(h, hipMemsetAsync(h->hist + (size_t)first * kHist, 0, sizeof(float2) * kHist * (size_t)count, 0));
        HIP_TRY(h, hipMemsetAsync(h->hist_far + (size_t)first * (kGenHist - kHist), 0, sizeof(float2) * (kGenHist - kHist) * (size_t)count, 0));
        // "all visible" = the longest delay line any kernel keeps (128); the regular rows saturate the count at their own 80
        hipLaunchKernelGGL(k_fill_i32, dim3((count + 255) / 256), dim3(256), 0, 0, h->rrc_valid + first, (int)kGenHist, count);
        HIP_TRY(h, hipGetLastError());
    } else {
        HIP_TRY(h, hipMemsetAsync(h->rrc_valid + first, 0, sizeof(int) * count, 0));
    }
    if ((rc = reset_timing(h, first, count))) return rc;
    HIP_TRY(h, hipMemsetAsync(h->cph + first, 0, sizeof(float) * count, 0));
    HIP_TRY(h, hipMemsetAsync(h->cfr + first, 0, sizeof(float) * count, 0));
    if (fresh) {
        // not touched by the reference's reset: ph2 (a plain member, pi4dqpsk_costas.h:32), the slicer's previous symbol
        // and statistic (DQPSKSymbolExtractor is another block), COMPLEX_FD's delay buffer
        HIP_TRY(h, hipMemsetAsync(h->ph2 + first, 0, sizeof(float) * count, 0));
        HIP_TRY(h, hipMemsetAsync(h->prev + first, 0, sizeof(int) * count, 0));
        if (h->q_ring) {
            HIP_TRY(h, hipMemsetAsync(h->q_ring + (size_t)first * 4096, 0, sizeof(float) * 4096 * (size_t)count, 0));
            HIP_TRY(h, hipMemsetAsync(h->q_ptr + first, 0, sizeof(int) * count, 0));
            HIP_TRY(h, hipMemsetAsync(h->q_disp + first, 0, sizeof(int) * count, 0));
            HIP_TRY(h, hipMemsetAsync(h->q_sync + first, 0, sizeof(int) * count, 0));
            HIP_TRY(h, hipMemsetAsync(h->q_err + first, 0, sizeof(float) * count, 0));
        }
        if (h->cd_blk) {                // (the Reshaper behind the symbol stream is another block too)
            HIP_TRY(h, hipMemsetAsync(h->cd_blk + (size_t)first * kCdSyms, 0, sizeof(float2) * kCdSyms * (size_t)count, 0));
            HIP_TRY(h, hipMemsetAsync(h->cd_fill + first, 0, sizeof(int) * count, 0));
            HIP_TRY(h, hipMemsetAsync(h->cd_blocks + first, 0, sizeof(int) * count, 0));
        }
        HIP_TRY(h, hipMemsetAsync(h->ybuf + (size_t)first * kYHist, 0, sizeof(float2) * kYHist * (size_t)count, 0));
    }
    HIP_TRY(h, hipStreamSynchronize(0));
    return TETRA_OK;
}

// Reads the kernels' overrun counter (the device must be idle for this handle's work) and tells whether it moved since the
// last report: > 0 = channels newly cut off, 0 = none, < 0 = a TETRA_ERR_* status.
int new_overruns(tetra_demod* h) {
    int total = 0;
    HIP_TRY(h, hipMemcpy(&total, h->d_overruns, sizeof(int), hipMemcpyDeviceToHost));
    const long long fresh = (long long)total - h->overruns_seen;
    h->overruns_seen = total;
    return fresh > 0 ? (int)(fresh > 0x7fffffff ? 0x7fffffff : fresh) : 0;
}

// The generic kernel's HBM scratch -- 2 x 8 B x C x (max_samples + 128), the delay lines of a whole call -- is held exactly while
// the plan says k_generic: allocated by create / the setter that moves the handle there (so that the stream-asynchronous process
// entry point never allocates or synchronises), released by the setter that moves it away.  The device is idle when this runs.
int sync_generic_scratch(tetra_demod* h, const host::LaunchPlan& plan) {
    if (!plan.generic) {
        h->g_xs.reset();
        h->g_ys.reset();
        return TETRA_OK;
    }
    const size_t xs_stride = (size_t)kGenHist + (size_t)h->max_samples, ys_stride = (size_t)kYHist + (size_t)h->max_samples;
    hipError_t e = h->g_xs.reserve(sizeof(float2) * xs_stride * (size_t)h->C);
    if (e == hipSuccess) e = h->g_ys.reserve(sizeof(float2) * ys_stride * (size_t)h->C);
    if (e != hipSuccess) {
        h->last_hip = (int)e;
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? TETRA_ERR_NOMEM : TETRA_ERR_HIP;
    }
    return TETRA_OK;
}

// Commits a design: the handle's parameters and its launch plan follow it, the generic kernel's scratch is allocated (a failure leaves
// the handle as it was) or, when the parameters have left that kernel's domain, released.
int commit_design(tetra_demod* h, const host::DesignParams& np, const host::Design& nd) {
    const host::LaunchPlan plan = host::plan_launch(h->C, h->cus, h->cfg.flags, nd);
    const int rc = sync_generic_scratch(h, plan);
    if (rc != TETRA_OK) return rc;
    h->dp = np;
    h->design = nd;
    h->plan = plan;
    return TETRA_OK;
}

// FIR::setTaps with more taps keeps the RRC's old taps-1 history samples and zero-fills the newly visible part (quirks handles)
int shrink_rrc_valid(tetra_demod* h, int old_ntaps) {
    if (!h->quirks || h->design.ntaps <= old_ntaps) return TETRA_OK;
    hipLaunchKernelGGL(k_min_i32, dim3((h->C + 255) / 256), dim3(256), 0, 0, h->rrc_valid, old_ntaps - 1, h->C);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(0));
    return TETRA_OK;
}

// "Let the asynchronous calls still in flight finish" (they run on their own three streams; state order)
int drain_async(tetra_demod* h) {
    if (!h->as.ready) return TETRA_OK;
    for (Stream* st : { &h->as.s_in, &h->as.s_k, &h->as.s_out }) HIP_TRY(h, hipStreamSynchronize(*st));
    return TETRA_OK;
}

// the handle's own (non-blocking) stream, created on first use
int ensure_own_stream(tetra_demod* h) {
    if (!h->own_stream) HIP_TRY(h, hipStreamCreateWithFlags(h->own_stream.put(), hipStreamNonBlocking));
    return TETRA_OK;
}

static_assert(host::kPlanCh == kFCh && host::kPlanChWide == kFChWide && host::kPlanChSmall == kFChSmall,
              "launch_plan.hpp plans the workgroup shapes kernel_fused.hpp has");

// What GenericParams and FusedParams have in common (same members, same names): the call's input and outputs, the channels' state,
// the loop constants.  Each kernel's own tables and extras are its caller's.
template <class P> void fill_common_params(P& p, const tetra_demod* h, const float* d_iq, int n_samples, uint8_t* d_bits, int bits_stride,
                                           int32_t* d_n_bits, float* d_sym) {
    p.iq = reinterpret_cast<const float2*>(d_iq);
    if (h->cfg.layout == TETRA_LAYOUT_CHANNEL_MAJOR) { p.in_ch_stride = n_samples; p.in_t_stride = 1; }
    else { p.in_ch_stride = 1; p.in_t_stride = h->C; }
    p.n = n_samples; p.n_channels = h->C;
    p.agc_g = h->agc_g; p.fll_ph = h->fll_ph; p.fll_fr = h->fll_fr; p.hist = h->hist;
    p.rrc_valid = h->rrc_valid;
    p.mu = h->mu; p.omega = h->omega; p.offset = h->offset;
    p.cph = h->cph; p.cfr = h->cfr; p.ph2 = h->ph2; p.prev = h->prev; p.ybuf = h->ybuf;
    p.ntaps = h->design.ntaps;
    p.bank = h->d_bank;
    p.bits = d_bits; p.bits_stride = bits_stride; p.n_bits = d_n_bits;
    p.sym = reinterpret_cast<float2*>(d_sym); p.sym_stride = bits_stride / 2;
    if (h->taps_sym() && !p.sym) { p.sym = h->q_sym; p.sym_stride = h->q_sym_stride; }      // a post-launch kernel reads the symbols
    p.y_dbg = h->keep_y ? h->y : nullptr;
    p.overruns = h->d_overruns;
    p.k1 = h->design.k1; p.k2 = h->design.k2;
}

// One launch of k_fused<true, false, CH, DEEP, LONG> over channels [first, first + count).
template <int CH, int DEEP, bool LONG>
void launch_fused(const tetra_demod* h, const FusedParams& pf, int first, int count, bool far_was_valid, hipStream_t s) {
    typename FusedArgs<CH, LONG>::type p;
    static_cast<FusedParams&>(p) = pf;
    p.ch_base = first;
    if constexpr (CH == kFChSmall) p.cut_flag4 = h->cut_flag;
    if constexpr (LONG) {      // the long rows also carry the 48 delay-line samples in front of hist's 80
        p.hist_far = h->hist_far;
        p.far_valid = far_was_valid ? 1 : 0;
    }
    hipLaunchKernelGGL((k_fused<true, false, CH, DEEP, LONG>), dim3((count + CH - 1) / CH), dim3(fused_threads(CH)), 0, s, p);
}

// The launches of a fused call as the plan says: channels [0, n_wide) in 32-channel workgroups, the rest in 16- or 4-channel ones -- at
// most two, back to back on the stream.  Exactly the instantiations that exist: the deep symbol ring's first level for the 16- and
// 4-channel shapes, its second for the 4-channel shape, none for the 32-channel shape (plan_launch never asks for another).
bool launch_fused_plan(const tetra_demod* h, const FusedParams& pf, hipStream_t s) {
    const host::LaunchPlan& plan = h->plan;
    const int first = plan.n_wide, count = h->C - first;
    if (first > 0) launch_fused<kFChWide, 0, false>(h, pf, 0, first, h->far_valid, s);
    if (count == 0) return true;
    constexpr auto key = [](int ch, int deep, bool long_rows) { return ch * 8 + deep * 2 + (long_rows ? 1 : 0); };
#define TETRA_REST(CH, DEEP, LONG) case key(CH, DEEP, LONG): launch_fused<CH, DEEP, LONG>(h, pf, first, count, h->far_valid, s); return true
    switch (key(plan.rest_ch, plan.deep, plan.long_rows)) {
    TETRA_REST(kFChSmall, 2, true); TETRA_REST(kFChSmall, 1, true); TETRA_REST(kFChSmall, 0, true);
    TETRA_REST(kFChSmall, 2, false); TETRA_REST(kFChSmall, 1, false); TETRA_REST(kFChSmall, 0, false);
    TETRA_REST(kFCh, 1, true); TETRA_REST(kFCh, 0, true);
    TETRA_REST(kFCh, 1, false); TETRA_REST(kFCh, 0, false);
    default: return false;
    }
#undef TETRA_REST
}

}  // namespace

extern "C" {

int tetra_demod_abi_version(void) { return TETRA_DEMOD_ABI_VERSION; }

// sha256 of the sources + flags this library was compiled from (build.py: source_hash() -> -DTETRA_BUILD_ID); the marker in
// front lets build.py read it from the file without loading it.
#ifndef TETRA_BUILD_ID
#define TETRA_BUILD_ID "0000000000000000000000000000000000000000000000000000000000000000"
#endif
const char* tetra_demod_build_id(void) {
    static const char id[] = "TETRA_BUILD_ID=" TETRA_BUILD_ID;
    return id + 15;
}

int tetra_demod_device_info(int device, int* clock_khz, int* compute_units) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return TETRA_ERR_NO_DEVICE;
    int v = 0;
    if (clock_khz) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeClockRate, device) != hipSuccess) return TETRA_ERR_HIP;
        *clock_khz = v;
    }
    if (compute_units) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return TETRA_ERR_HIP;
        *compute_units = v;
    }
    return TETRA_OK;
}

const char* tetra_demod_strerror(int status) {
    switch (status) {
    case TETRA_OK: return "ok";
    case TETRA_ERR_ARG: return "invalid argument";
    case TETRA_ERR_UNSUPPORTED: return "unsupported parameter";
    case TETRA_ERR_NO_DEVICE: return "no usable HIP device";
    case TETRA_ERR_HIP: return "HIP runtime error";
    case TETRA_ERR_NOMEM: return "out of memory";
    case TETRA_ERR_SIZE: return "size out of range";
    case TETRA_ERR_ALIGN: return "misaligned output buffer";
    case TETRA_ERR_OVERRUN: return "a channel filled its output row and was cut off (outputs delivered)";
    default: return "unknown status";
    }
}

int tetra_demod_default_config(tetra_demod_config_t* cfg) {
    if (!cfg) return TETRA_ERR_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_channels = 1;
    cfg->max_samples = 65536;
    cfg->layout = TETRA_LAYOUT_CHANNEL_MAJOR;
    cfg->device = -1;
    cfg->symbolrate = 18000;
    cfg->samplerate = 36000;
    cfg->rrc_tap_count = 65;
    cfg->rrc_beta = 0.35f;
    cfg->agc_rate = 0.02f;
    cfg->costas_bandwidth = 0.01f;
    cfg->fll_bandwidth = 0.006f;
    host::default_timing_gains(cfg->omega_gain, cfg->mu_gain);
    cfg->omega_rel_limit = 0.02f;
    return TETRA_OK;
}

int tetra_demod_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int tetra_demod_bits_stride(int n_samples) {
    if (n_samples < 0) return TETRA_ERR_ARG;
    // bits = 2 * symbols; n / 0.95 + 16 covers every timing loop whose slowest step is >= 1.9 samples per symbol
    // (tetra_demod_bits_stride_for: the reference plugin's parameters give 1.9424)
    long long s = (long long)((double)n_samples / 0.95) + 16;
    s = (s + 15) / 16 * 16;
    return s > 0x7ffffff0ll ? TETRA_ERR_SIZE : (int)s;
}

namespace {
long long stride_for(const host::Design& d, long long n) { return host::bits_stride_for(d, n); }
}  // namespace

int tetra_demod_bits_stride_for(tetra_demod_t* h, int n_samples) {
    if (!h || n_samples < 0) return TETRA_ERR_ARG;
    const long long s = stride_for(h->design, n_samples);
    return s > 0x7ffffff0ll ? TETRA_ERR_SIZE : (int)s;
}

int tetra_demod_create(const tetra_demod_config_t* cfg, tetra_demod_t** out) {
    if (!cfg || !out) return TETRA_ERR_ARG;
    *out = nullptr;
    if (cfg->n_channels < 1 || cfg->max_samples < 1) return TETRA_ERR_ARG;
    if (cfg->layout != TETRA_LAYOUT_CHANNEL_MAJOR && cfg->layout != TETRA_LAYOUT_TIME_MAJOR) return TETRA_ERR_ARG;
    {
        const int shapes = cfg->flags & (TETRA_FLAG_WIDE_WORKGROUPS | TETRA_FLAG_NARROW_WORKGROUPS | TETRA_FLAG_SMALL_WORKGROUPS);
        if (shapes & (shapes - 1)) return TETRA_ERR_ARG;      // at most one shape can be forced
    }
    int ndev = tetra_demod_device_count();
    if (ndev <= 0) return TETRA_ERR_NO_DEVICE;
    int dev = cfg->device;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return TETRA_ERR_NO_DEVICE;
    }
    if (dev >= ndev) return TETRA_ERR_NO_DEVICE;

    tetra_demod* h = new (std::nothrow) tetra_demod();
    if (!h) return TETRA_ERR_NOMEM;
    h->cfg = *cfg;
    h->cfg.rrc_taps = h->cfg.bandedge_taps = h->cfg.interp_bank = nullptr;
    h->device = dev;
    h->C = cfg->n_channels;
    h->max_samples = cfg->max_samples;
    h->dp.symbolrate = cfg->symbolrate;
    h->dp.samplerate = cfg->samplerate;
    h->dp.rrc_tap_count = cfg->rrc_tap_count;
    h->dp.rrc_beta = cfg->rrc_beta;
    h->dp.agc_rate = cfg->agc_rate;
    h->dp.costas_bandwidth = cfg->costas_bandwidth;
    h->dp.fll_bandwidth = cfg->fll_bandwidth;
    h->dp.omega_gain = cfg->omega_gain;
    h->dp.mu_gain = cfg->mu_gain;
    h->dp.omega_rel_limit = cfg->omega_rel_limit;
    if (!host::make_design(h->dp, cfg->rrc_taps, cfg->bandedge_taps, cfg->interp_bank, h->design) ||
        stride_for(h->design, cfg->max_samples) > 0x7ffffff0ll || (cfg->flags & TETRA_FLAG_RETIRED_TWO_KERNEL)) {
        delete h;
        return TETRA_ERR_UNSUPPORTED;
    }
    DeviceGuard g(dev);
    if (!g.ok) {
        delete h;
        return TETRA_ERR_NO_DEVICE;
    }
    const size_t C = (size_t)h->C;
    int rc = TETRA_OK;
    auto A = [&](auto& buf, size_t count) {      // every allocation is attempted; the first failure is the status
        const hipError_t e = buf.reserve(sizeof(*buf.get()) * count);
        if (e != hipSuccess) { h->last_hip = (int)e; if (rc == TETRA_OK) rc = TETRA_ERR_HIP; }
    };
    A(h->agc_g, C); A(h->fll_ph, C); A(h->fll_fr, C);
    A(h->hist, C * kHist);
    A(h->hist_far, C * (size_t)(kGenHist - kHist));
    A(h->d_g_be_a, (size_t)kGenMaxTaps); A(h->d_g_be_b, (size_t)kGenMaxTaps); A(h->d_g_rrc, (size_t)kGenMaxTaps);
    A(h->mu, C); A(h->omega, C); A(h->cph, C); A(h->cfr, C);
    A(h->ph2, C); A(h->offset, C); A(h->prev, C);
    A(h->rrc_valid, C);
    h->user_rrc = cfg->rrc_taps != nullptr;
    h->user_be = cfg->bandedge_taps != nullptr;
    h->quirks = (cfg->flags & TETRA_FLAG_REFERENCE_QUIRKS) != 0;
    h->keep_y = (cfg->flags & TETRA_FLAG_KEEP_RRC_OUT) != 0;
    (void)hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (h->cus <= 0) h->cus = 256;
    h->plan = host::plan_launch(h->C, h->cus, cfg->flags, h->design);
    if (h->keep_y) A(h->y, C * ((size_t)h->max_samples + kYHist));
    A(h->ybuf, C * kYHist);
    if (cfg->flags & TETRA_FLAG_QUALITY) {
        A(h->q_ring, C * 4096); A(h->q_ptr, C);
        A(h->q_disp, C); A(h->q_sync, C); A(h->q_err, C);
    }
    if (cfg->flags & TETRA_FLAG_CONSTELLATION) {
        A(h->cd_blk, C * (size_t)kCdSyms); A(h->cd_part, C * (size_t)kCdSyms);
        A(h->cd_fill, C); A(h->cd_blocks, C);
    }
    if (cfg->flags & (TETRA_FLAG_QUALITY | TETRA_FLAG_CONSTELLATION)) {
        h->q_sym_stride = stride_for(h->design, h->max_samples) / 2;
        A(h->q_sym, C * (size_t)h->q_sym_stride);
    }
    A(h->d_overruns, (size_t)1);
    A(h->d_be_re80, (size_t)kBePadLong); A(h->d_be_im80, (size_t)kBePadLong);   // (sized for the long rows' tables)
    A(h->d_rrc_ext, (size_t)kRrcExtLong);
    A(h->d_bank, (size_t)kInterpPhases * kInterpTaps);
    if (rc == TETRA_OK && hipMemset(h->d_overruns, 0, sizeof(int)) != hipSuccess) rc = TETRA_ERR_HIP;
    for (auto& slot : h->ev)
        for (auto& e : slot)
            if (rc == TETRA_OK && hipEventCreate(e.put()) != hipSuccess) rc = TETRA_ERR_HIP;
    if (rc == TETRA_OK) rc = upload_tables(h);
    if (rc == TETRA_OK) rc = reset_range(h, 0, h->C, true);
    if (rc == TETRA_OK) rc = sync_generic_scratch(h, h->plan);
    if (rc != TETRA_OK) {
        int st = (h->last_hip == (int)hipErrorOutOfMemory) ? TETRA_ERR_NOMEM : rc;
        delete h;
        return st;
    }
    *out = h;
    return TETRA_OK;
}

int tetra_demod_destroy(tetra_demod_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return TETRA_OK;
}

int tetra_demod_process_device(tetra_demod_t* h, const float* d_iq, int n_samples, uint8_t* d_bits, int bits_stride,
                               int32_t* d_n_bits, float* d_sym, void* hip_stream) {
    if (!h || !d_iq || !d_bits || !d_n_bits) return TETRA_ERR_ARG;
    if (n_samples < 0 || n_samples > h->max_samples) return TETRA_ERR_SIZE;
    if (bits_stride < stride_for(h->design, n_samples)) return TETRA_ERR_SIZE;
    if ((bits_stride & 7) || (reinterpret_cast<uintptr_t>(d_bits) & 7) || (reinterpret_cast<uintptr_t>(d_sym) & 7))
        return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)hip_stream;
    h->last_n = n_samples;
    if (n_samples == 0) {
        HIP_TRY(h, hipMemsetAsync(d_n_bits, 0, sizeof(int32_t) * (size_t)h->C, s));
        return TETRA_OK;
    }
    const host::LaunchPlan& plan = h->plan;
    const Event* ev = h->ev[h->n_calls % tetra_demod::kEvSlots];
    GenericParams pg;
    FusedParams pf;
#ifdef TETRA_DEMOD_DEBUG
    // Debug builds only (profiles/build_debug.sh): TETRA_DEMOD_PROFILE=<file> appends the per-role busy clocks of every
    // launch to <file>.  The release library has neither the getenv nor the instrumented instantiation.
    const char* prof_path = std::getenv("TETRA_DEMOD_PROFILE");
    const size_t prof_wgs = (size_t)(h->C + kFCh - 1) / kFCh;
    bool profiling = false;
#endif
    if (plan.generic) {
        // one lane per channel, delay lines in an HBM scratch (kernel_generic.hpp) that create / the setters hold ready (sync_generic_scratch)
        if (!h->g_xs || !h->g_ys) return TETRA_ERR_NOMEM;
        fill_common_params(pg, h, d_iq, n_samples, d_bits, bits_stride, d_n_bits, d_sym);
        pg.hist_far = h->hist_far; pg.far_valid = h->far_valid ? 1 : 0;
        pg.be_a = h->d_g_be_a; pg.be_b = h->d_g_be_b; pg.rrc = h->d_g_rrc; pg.ntaps_be = h->design.ntaps_be;
        pg.xs = h->g_xs; pg.ys = h->g_ys;
        pg.xs_stride = (long long)kGenHist + h->max_samples; pg.ys_stride = (long long)kYHist + h->max_samples;
        pg.cut_flag = h->cut_flag;
        pg.lanes = host::generic_lanes(h->C, h->cus);
    } else {
        fill_common_params(pf, h, d_iq, n_samples, d_bits, bits_stride, d_n_bits, d_sym);
        pf.ch_base = 0;
        pf.be_re80 = h->d_be_re80; pf.be_im80 = h->d_be_im80; pf.rrc_ext = h->d_rrc_ext;
        pf.prof = reinterpret_cast<long long*>(h->cut_flag);      // the non-instrumented 16- / 32-channel kernels read it as the cut flag (kernel_fused.hpp)
        // the FLL's loop filter runs with alpha = 0 (fll.cpp:25; design.hpp never produces anything else): only those kernels exist
        if (pf.k1.fll_alpha != 0.0f) return TETRA_ERR_UNSUPPORTED;
#ifdef TETRA_DEMOD_DEBUG
        if (prof_path && plan.n_wide == 0 && plan.rest_ch == kFCh && !plan.long_rows) {      // (the instrumented instantiation exists for the regular rows only)
            if (!h->d_prof) HIP_TRY(h, h->d_prof.reserve(sizeof(long long) * 8 * prof_wgs));
            HIP_TRY(h, hipMemsetAsync(h->d_prof, 0, sizeof(long long) * 8 * prof_wgs, s));
            pf.prof = h->d_prof;
            profiling = true;
        }
#endif
    }
    HIP_TRY(h, hipEventRecord(ev[0], s));
    if (plan.generic) {
        hipLaunchKernelGGL(k_generic, dim3((h->C + pg.lanes - 1) / pg.lanes), dim3(64), 0, s, pg);
    } else {
#ifdef TETRA_DEMOD_DEBUG
        if (profiling && !plan.deep) {
            FusedParamsT<kFCh> pp;
            static_cast<FusedParams&>(pp) = pf;
            hipLaunchKernelGGL((k_fused<true, true>), dim3(prof_wgs), dim3(kFThreads), 0, s, pp);
        } else
#endif
        if (!launch_fused_plan(h, pf, s)) return TETRA_ERR_UNSUPPORTED;
    }
    const float2* sym = plan.generic ? pg.sym : pf.sym;      // where the launch leaves its symbols: the taps behind it read them
    const long long sym_stride = plan.generic ? pg.sym_stride : pf.sym_stride;
    if (h->q_ring)
        hipLaunchKernelGGL(k_quality, dim3(h->C), dim3(64), 0, s, sym, sym_stride, d_n_bits, h->q_ring, h->q_ptr, h->q_disp,
                           h->q_err, h->q_sync);
    if (h->cd_blk)
        hipLaunchKernelGGL(k_constellation, dim3(h->C), dim3(256), 0, s, sym, sym_stride, d_n_bits, h->cd_blk, h->cd_part,
                           h->cd_fill, h->cd_blocks);
    HIP_TRY(h, hipGetLastError());
    // the generic kernel carries all 128 delay-line samples, the fused kernel the newest 80 only -- its long rows all 128
    h->far_valid = plan.generic || plan.long_rows;
    HIP_TRY(h, hipEventRecord(ev[1], s));
    h->n_calls++;
#ifdef TETRA_DEMOD_DEBUG
    if (profiling) {
        const size_t nwg = prof_wgs;
        std::vector<long long> host(8 * nwg);
        HIP_TRY(h, hipStreamSynchronize(s));
        HIP_TRY(h, hipMemcpy(host.data(), h->d_prof, sizeof(long long) * host.size(), hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(prof_path, "a")) {
            double sum[8] = { 0 };
            for (size_t w = 0; w < nwg; w++)
                for (int r = 0; r < 8; r++) sum[r] += (double)host[8 * w + r];
            std::fprintf(f, "{\"n\": %d, \"workgroups\": %zu, \"mean_busy_clocks\": {\"E\": %.0f, \"D\": %.0f, \"F0\": %.0f, \"F1\": %.0f, \"A\": %.0f, \"C\": %.0f}, \"mean_total_clocks\": %.0f}\n",
                         n_samples, nwg, sum[0] / nwg, sum[1] / nwg, sum[2] / nwg, sum[3] / nwg, sum[4] / nwg, sum[5] / nwg, sum[7] / nwg);
            std::fclose(f);
        }
    }
#endif
    return TETRA_OK;
}

int tetra_demod_process_resident(tetra_demod_t* h, const float* d_iq, int n_samples, uint8_t* d_bits, int bits_stride,
                                 int32_t* d_n_bits, float* d_sym) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    int rc;
    if ((rc = drain_async(h)) || (rc = ensure_own_stream(h))) return rc;
    rc = tetra_demod_process_device(h, d_iq, n_samples, d_bits, bits_stride, d_n_bits, d_sym, h->own_stream);
    if (rc != TETRA_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->own_stream));
    const int cut = new_overruns(h);
    return cut > 0 ? TETRA_ERR_OVERRUN : cut;
}

int tetra_demod_process(tetra_demod_t* h, const float* iq, int n_samples, uint8_t* bits, int bits_stride,
                        int32_t* n_bits, float* sym) {
    if (!h || !iq || !bits || !n_bits) return TETRA_ERR_ARG;
    if (n_samples < 0 || n_samples > h->max_samples) return TETRA_ERR_SIZE;
    if (bits_stride < stride_for(h->design, n_samples)) return TETRA_ERR_SIZE;
    if (bits_stride & 7) return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    int rc;
    if ((rc = drain_async(h))) return rc;
    const size_t C = (size_t)h->C;
    const size_t iq_bytes = sizeof(float) * 2 * C * (size_t)n_samples;
    const size_t bits_bytes = C * (size_t)bits_stride;
    const size_t sym_bytes = sym ? sizeof(float) * 2 * C * (size_t)(bits_stride / 2) : 0;
    // Small calls -- the single-channel drop-in hands over 180 samples at a time (SDR++'s stream chunks at 36 ksps) -- are
    // dominated by the four blocking copies around a ~40 us launch.  They take one asynchronous chain on the handle's own
    // stream instead: samples through a page-locked bounce buffer, ONE packed output [n_bits | bits | symbols] back into
    // page-locked memory, one synchronisation, then plain memcpys into the caller's arrays.
    constexpr size_t kSmallCall = 256 * 1024;
    const size_t nb_bytes = (sizeof(int) * C + 15) / 16 * 16;
    const size_t pack_bytes = nb_bytes + bits_bytes + sym_bytes + 16;      // + the overrun counter, so that it rides along
#ifdef TETRA_EXP_TINY_ENV      // experiment builds: the in-place limit from the environment (profiles/measure_tiny_calls.py)
    static const int kTiny = std::getenv("TETRA_TINY_SAMPLES") ? std::atoi(std::getenv("TETRA_TINY_SAMPLES")) : kTinyCallSamples;
#else
    constexpr int kTiny = kTinyCallSamples;
#endif
    const bool small_call = n_samples > 0 && iq_bytes <= kSmallCall && pack_bytes <= kSmallCall;
    if (small_call && (rc = ensure_own_stream(h))) return rc;
    bool tiny = small_call && n_samples <= kTiny && !h->tn_disabled;
    if (tiny) {
        // The shortest calls use no copy engine at all: the CPU copies the samples into a page-locked, mapped, coherent block
        // that the AGC wave reads in place over PCIe (a tile ahead, as always), the kernels write n_bits | bits | symbols | a
        // "some channel was cut off" flag straight into a second such block, ONE synchronisation, plain memcpys out.  Measured
        // (profiles/r03/r03_ad_tiny_calls.json): 1 x 180 samples 67.7 -> 59.9 us per call, 16 x 180 77.6 -> 62.7, 64 x 180
        // 88.0 -> 65.9, 64 x 500 128.7 -> 109.4; the launch itself gets ~10 % slower per sample (the AGC wave's loads cross
        // PCIe), which is why calls of more than kTinyCallSamples keep the copy engines (1 x 1024: 144 vs 147 us).
        // The overrun COUNTER stays in device memory (an atomic across PCIe is not something every platform routes); a channel
        // that is cut off additionally leaves a plain store in the host block, and only then is the counter read back.
        // A platform that refuses mapped + coherent host memory (or its device pointer) loses nothing but this shortcut: the
        // blocks are only kept once BOTH calls succeeded, otherwise the path is switched off and the call continues below.
        auto mapped_block = [&](HostMem<uint8_t>& host_p, uint8_t** dev_p) {
            if (host_p) return true;
            HostMem<uint8_t> hp;
            uint8_t* dp = nullptr;
            if (hp.reserve(kSmallCall, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return false; }
            if (hipHostGetDevicePointer((void**)&dp, hp, 0) != hipSuccess || !dp) { (void)hipGetLastError(); return false; }
            std::memset(hp, 0, kSmallCall);
            host_p = std::move(hp); *dev_p = dp;
            return true;
        };
        if (!mapped_block(h->tn_out, &h->tn_out_dev) || !mapped_block(h->tn_in, &h->tn_in_dev)) h->tn_disabled = true;
        tiny = !h->tn_disabled;
    }
    if (tiny) {
        std::memcpy(h->tn_in, iq, iq_bytes);
        volatile int* flag = reinterpret_cast<volatile int*>(h->tn_out + pack_bytes - 16);
        *flag = 0;
        uint8_t* d_bits = h->tn_out_dev + nb_bytes;
        h->cut_flag = reinterpret_cast<int*>(h->tn_out_dev + pack_bytes - 16);
        rc = tetra_demod_process_device(h, reinterpret_cast<const float*>(h->tn_in_dev), n_samples, d_bits, bits_stride,
                                        reinterpret_cast<int32_t*>(h->tn_out_dev), sym ? reinterpret_cast<float*>(d_bits + bits_bytes) : nullptr,
                                        h->own_stream);
        h->cut_flag = nullptr;
        if (rc != TETRA_OK) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->own_stream));
        std::memcpy(n_bits, h->tn_out, sizeof(int) * C);
        std::memcpy(bits, h->tn_out + nb_bytes, bits_bytes);
        if (sym) std::memcpy(sym, h->tn_out + nb_bytes + bits_bytes, sym_bytes);
        if (*flag == 0) return TETRA_OK;
        const int cut = new_overruns(h);          // rare: a poisoned channel filled its row
        return cut < 0 ? cut : TETRA_ERR_OVERRUN;
    }
    if (small_call) {
        if (!h->pk_host) {      // once, both at kSmallCall; the packed output starts zero-filled
            HIP_TRY(h, h->pk_dev.reserve(kSmallCall));
            HIP_TRY(h, hipMemset(h->pk_dev, 0, kSmallCall));
            HIP_TRY(h, h->pk_host.reserve(kSmallCall));
        }
        HIP_TRY(h, h->pk_in.reserve(kSmallCall));
        HIP_TRY(h, h->st_iq.reserve(iq_bytes));
        std::memcpy(h->pk_in, iq, iq_bytes);
        HIP_TRY(h, hipMemcpyAsync(h->st_iq, h->pk_in, iq_bytes, hipMemcpyHostToDevice, h->own_stream));
        uint8_t* d_nb = h->pk_dev;
        uint8_t* d_bits = h->pk_dev + nb_bytes;
        uint8_t* d_sym = d_bits + bits_bytes;
        rc = tetra_demod_process_device(h, h->st_iq, n_samples, d_bits, bits_stride, reinterpret_cast<int32_t*>(d_nb),
                                        sym ? reinterpret_cast<float*>(d_sym) : nullptr, h->own_stream);
        if (rc != TETRA_OK) return rc;
        HIP_TRY(h, hipMemcpyAsync(h->pk_dev + pack_bytes - 16, h->d_overruns, sizeof(int), hipMemcpyDeviceToDevice, h->own_stream));
        HIP_TRY(h, hipMemcpyAsync(h->pk_host, h->pk_dev, pack_bytes, hipMemcpyDeviceToHost, h->own_stream));
        HIP_TRY(h, hipStreamSynchronize(h->own_stream));
        std::memcpy(n_bits, h->pk_host, sizeof(int) * C);
        std::memcpy(bits, h->pk_host + nb_bytes, bits_bytes);
        if (sym) std::memcpy(sym, h->pk_host + nb_bytes + bits_bytes, sym_bytes);
        int total = 0;
        std::memcpy(&total, h->pk_host + pack_bytes - 16, sizeof(int));
        const long long fresh = (long long)total - h->overruns_seen;
        h->overruns_seen = total;
        return fresh > 0 ? TETRA_ERR_OVERRUN : TETRA_OK;
    }
    HIP_TRY(h, h->st_iq.reserve(iq_bytes));
    if (bits_bytes > h->st_bits.bytes()) {      // once per size: the kernels define bits[c][0 .. n_bits[c]) per call, the rest stays as it is
        HIP_TRY(h, h->st_bits.reserve(bits_bytes));
        const hipError_t e = hipMemset(h->st_bits, 0, bits_bytes);
        if (e != hipSuccess) h->st_bits.reset();      // (kept only zero-filled)
        HIP_TRY(h, e);
    }
    HIP_TRY(h, h->st_nbits.reserve(sizeof(int) * C));
    HIP_TRY(h, h->st_sym.reserve(sym_bytes));
    if (iq_bytes) HIP_TRY(h, hipMemcpy(h->st_iq, iq, iq_bytes, hipMemcpyHostToDevice));
#ifdef TETRA_DEMOD_DEBUG
    HIP_TRY(h, hipMemset(h->st_bits, 0, bits_bytes));      // release builds: only bits[c][0 .. n_bits[c]) are defined
#endif
    rc = tetra_demod_process_device(h, h->st_iq ? h->st_iq : h->agc_g, n_samples, h->st_bits, bits_stride, h->st_nbits,
                                    sym ? h->st_sym.get() : nullptr, nullptr);
    if (rc != TETRA_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(0));
    HIP_TRY(h, hipMemcpy(bits, h->st_bits, bits_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(n_bits, h->st_nbits, sizeof(int) * C, hipMemcpyDeviceToHost));
    if (sym) HIP_TRY(h, hipMemcpy(sym, h->st_sym, sym_bytes, hipMemcpyDeviceToHost));
    const int cut = new_overruns(h);
    return cut > 0 ? TETRA_ERR_OVERRUN : cut;
}

// ------------------------------------------------------------------------------------------------
// Asynchronous host entry point.  The call is cut along the TIME axis into chunks (state carries from chunk to chunk like
// from call to call, so the bits are those of one call); chunk k+1 crosses PCIe while chunk k is demodulated:
//   s_in : H2D of chunk k into slot k%2                      (waits until the kernel that last read that slot is done)
//   s_k  : [int16 -> float] -> k_fused -> k_append_bits        (waits for the copy)
//   s_out: D2H of the call's bits and counts                   (waits for the last append)
// Two calls may be in flight (two output slots), so call j+1's input copy overlaps call j's output copy.
// ------------------------------------------------------------------------------------------------
namespace {
int async_chunk_len(int n_samples) {
    int k = n_samples / 4096;
    k = k < 1 ? 1 : (k > 8 ? 8 : k);
    const int len = (n_samples + k - 1) / k;
    return (len + 31) & ~31;
}
}  // namespace

namespace {
// The body of tetra_demod_process_async after its resources exist; any failure leaves work enqueued on the three streams.
int async_enqueue(tetra_demod* h, const void* iq, int iq_format, int n_samples, uint8_t* bits, int bits_stride, int32_t* n_bits) {
    auto& a = h->as;
    const size_t C = (size_t)h->C;
    const int chunk = async_chunk_len(n_samples);
    const int cstride = (int)stride_for(h->design, chunk);
    const size_t in_elem = iq_format == TETRA_IQ_CS16 ? sizeof(short) * 2 : iq_format == TETRA_IQ_CS8 ? 2 : sizeof(float) * 2;
    const size_t want_iq = sizeof(float) * 2 * C * (size_t)chunk, want_raw = iq_format != TETRA_IQ_CF32 ? in_elem * C * (size_t)chunk : 0;
    const size_t want_cbits = C * (size_t)cstride, want_out = C * (size_t)bits_stride;
    auto fits = [&](int i) {
        return a.d_iq[i].bytes() >= want_iq && a.d_raw[i].bytes() >= want_raw && a.d_cbits[i].bytes() >= want_cbits && a.d_out[i].bytes() >= want_out;
    };
    if (!fits(0) || !fits(1)) {
        HIP_TRY(h, hipDeviceSynchronize());          // buffers may be in use by calls still in flight
        for (int i = 0; i < 2; i++) {
            HIP_TRY(h, a.d_iq[i].reserve(want_iq));
            HIP_TRY(h, a.d_raw[i].reserve(want_raw));
            HIP_TRY(h, a.d_cbits[i].reserve(want_cbits));
            if (want_out > a.d_out[i].bytes()) {     // once per size; a call defines bits[c][0 .. n_bits[c])
                HIP_TRY(h, a.d_out[i].reserve(want_out));
                const hipError_t e = hipMemset(a.d_out[i], 0, want_out);
                if (e != hipSuccess) a.d_out[i].reset();      // (kept only zero-filled)
                HIP_TRY(h, e);
            }
        }
    }
    const int os = (int)(a.calls & 1);               // output slot of this call
    if (a.calls >= 2) HIP_TRY(h, hipStreamWaitEvent(a.s_k, a.ev_out[os], 0));     // its previous user's D2H is done
    HIP_TRY(h, hipMemsetAsync(a.d_onb[os], 0, sizeof(int) * C, a.s_k));
    const bool time_major = h->cfg.layout == TETRA_LAYOUT_TIME_MAJOR;
    const uint8_t* src = static_cast<const uint8_t*>(iq);
    for (int pos = 0; pos < n_samples; pos += chunk) {
        const int len = n_samples - pos < chunk ? n_samples - pos : chunk;
        const int sl = (int)(a.chunks & 1);
        if (a.chunks >= 2) HIP_TRY(h, hipStreamWaitEvent(a.s_in, a.ev_free[sl], 0));
        void* dst = iq_format != TETRA_IQ_CF32 ? a.d_raw[sl].get() : (void*)a.d_iq[sl].get();
        if (time_major) {      // iq[n][c]: a time chunk is contiguous
            HIP_TRY(h, hipMemcpyAsync(dst, src + in_elem * C * (size_t)pos, in_elem * C * (size_t)len, hipMemcpyHostToDevice, a.s_in));
        } else {               // iq[c][n]: one row piece per channel, packed to [C][len] on the device
            HIP_TRY(h, hipMemcpy2DAsync(dst, in_elem * (size_t)len, src + in_elem * (size_t)pos, in_elem * (size_t)n_samples,
                                        in_elem * (size_t)len, C, hipMemcpyHostToDevice, a.s_in));
        }
        HIP_TRY(h, hipEventRecord(a.ev_in[sl], a.s_in));
        HIP_TRY(h, hipStreamWaitEvent(a.s_k, a.ev_in[sl], 0));
        if (iq_format == TETRA_IQ_CS16) {
            const long long n = (long long)C * len;
            hipLaunchKernelGGL(k_cs16_to_cf32, dim3(2048), dim3(256), 0, a.s_k, static_cast<const short2*>(a.d_raw[sl].get()),
                               reinterpret_cast<float2*>(a.d_iq[sl].get()), n);
            HIP_TRY(h, hipGetLastError());
        } else if (iq_format == TETRA_IQ_CS8) {
            const long long n = (long long)C * len;
            hipLaunchKernelGGL(k_cs8_to_cf32, dim3(2048), dim3(256), 0, a.s_k, static_cast<const char2*>(a.d_raw[sl].get()),
                               reinterpret_cast<float2*>(a.d_iq[sl].get()), n);
            HIP_TRY(h, hipGetLastError());
        }
        const int rc = tetra_demod_process_device(h, a.d_iq[sl], len, a.d_cbits[sl], cstride, a.d_cnb[sl], nullptr, a.s_k);
        if (rc != TETRA_OK) return rc;
        hipLaunchKernelGGL(k_append_bits, dim3((unsigned)C), dim3(64), 0, a.s_k, a.d_cbits[sl], cstride, a.d_cnb[sl], a.d_out[os],
                           bits_stride, a.d_onb[os]);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipEventRecord(a.ev_free[sl], a.s_k));
        a.chunks++;
    }
    HIP_TRY(h, hipEventRecord(a.ev_done[os], a.s_k));
    HIP_TRY(h, hipStreamWaitEvent(a.s_out, a.ev_done[os], 0));
    HIP_TRY(h, hipMemcpyAsync(bits, a.d_out[os], want_out, hipMemcpyDeviceToHost, a.s_out));
    HIP_TRY(h, hipMemcpyAsync(n_bits, a.d_onb[os], sizeof(int) * C, hipMemcpyDeviceToHost, a.s_out));
    HIP_TRY(h, hipEventRecord(a.ev_out[os], a.s_out));
    a.calls++;
    return TETRA_OK;
}
}  // namespace

int tetra_demod_process_async(tetra_demod_t* h, const void* iq, int iq_format, int n_samples, uint8_t* bits, int bits_stride,
                              int32_t* n_bits) {
    if (!h || !iq || !bits || !n_bits) return TETRA_ERR_ARG;
    if (iq_format != TETRA_IQ_CF32 && iq_format != TETRA_IQ_CS16 && iq_format != TETRA_IQ_CS8) return TETRA_ERR_ARG;
    if (n_samples < 0 || n_samples > h->max_samples) return TETRA_ERR_SIZE;
    if (bits_stride < stride_for(h->design, n_samples)) return TETRA_ERR_SIZE;
    if (bits_stride & 7) return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    auto& a = h->as;
    const size_t C = (size_t)h->C;
    if (n_samples == 0) {      // nothing to enqueue: the counts are final right away
        for (size_t c = 0; c < C; c++) n_bits[c] = 0;
        return TETRA_OK;
    }
    if (!a.ready) {
        // every resource is created only where it is still missing, so a call after a failed set-up neither leaks nor
        // re-creates what already exists
        for (Stream* st : { &a.s_in, &a.s_k, &a.s_out })
            if (!*st) HIP_TRY(h, hipStreamCreateWithFlags(st->put(), hipStreamNonBlocking));
        for (int i = 0; i < 2; i++) {
            for (Event* e : { &a.ev_in[i], &a.ev_free[i], &a.ev_done[i], &a.ev_out[i] })
                if (!*e) HIP_TRY(h, hipEventCreateWithFlags(e->put(), hipEventDisableTiming));
            HIP_TRY(h, a.d_cnb[i].reserve(sizeof(int) * C));
            HIP_TRY(h, a.d_onb[i].reserve(sizeof(int) * C));
        }
        a.ready = true;
    }
    const int rc = async_enqueue(h, iq, iq_format, n_samples, bits, bits_stride, n_bits);
    if (rc != TETRA_OK) {
        // part of the call may be enqueued: let it drain, then start the slot / event bookkeeping afresh (no wait of a later
        // call refers to an event this call did not get to record)
        (void)drain_async(h);
        a.chunks = 0;
        a.calls = 0;
    }
    return rc;
}

int tetra_demod_wait(tetra_demod_t* h) {
    if (!h) return TETRA_ERR_ARG;
    if (!h->as.ready) return TETRA_OK;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    const int rc = drain_async(h);
    if (rc != TETRA_OK) return rc;
    const int cut = new_overruns(h);
    return cut > 0 ? TETRA_ERR_OVERRUN : cut;
}

int tetra_demod_get_overruns(tetra_demod_t* h, long long* total) {
    if (!h || !total) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    int v = 0;
    HIP_TRY(h, hipMemcpy(&v, h->d_overruns, sizeof(int), hipMemcpyDeviceToHost));
    *total = (long long)v;
    return TETRA_OK;
}

void* tetra_demod_host_alloc(size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}

void tetra_demod_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int tetra_demod_reset(tetra_demod_t* h, int channel) {
    if (!h) return TETRA_ERR_ARG;
    if (channel < -1 || channel >= h->C) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    return channel < 0 ? reset_range(h, 0, h->C, !h->quirks) : reset_range(h, channel, 1, !h->quirks);
}

}  // extern "C"

// The per-channel state that reset_range writes, for the stream-ordered reset of listed channels (tetra_retune.hip, retune_core.hpp)
int retune_impl::demod_view(tetra_demod_t* h, retune::DemodView* v) {
    if (!h || !v) return TETRA_ERR_ARG;
    *v = retune::DemodView{};
    v->agc_g = h->agc_g; v->fll_ph = h->fll_ph; v->fll_fr = h->fll_fr; v->mu = h->mu; v->omega = h->omega;
    v->cph = h->cph; v->cfr = h->cfr; v->ph2 = h->ph2; v->offset = h->offset; v->prev = h->prev; v->rrc_valid = h->rrc_valid;
    v->hist = reinterpret_cast<float*>(h->hist.get()); v->n_hist = kHist;
    v->hist_far = reinterpret_cast<float*>(h->hist_far.get()); v->n_hist_far = kGenHist - kHist;
    v->ybuf = reinterpret_cast<float*>(h->ybuf.get()); v->n_ybuf = kYHist;
    v->q_ring = h->q_ring; v->q_ptr = h->q_ptr; v->q_disp = h->q_disp; v->q_sync = h->q_sync; v->q_err = h->q_err; v->n_q_ring = 4096;
    v->cd_blk = reinterpret_cast<float*>(h->cd_blk.get()); v->cd_fill = h->cd_fill; v->cd_blocks = h->cd_blocks; v->n_cd = kCdSyms;
    v->rrc_all = kGenHist;
    v->tr_omega = h->design.tr_omega;
    v->fresh = h->quirks ? 0 : 1;
    return TETRA_OK;
}

extern "C" {

namespace {
// What every setter ends in: validate the new parameter set, re-design what `tables` / `with_tap_count` ask for, then commit
// (device tables, the RRC's view of a longer delay line, the timing loop, the statistic's symbol scratch).
int apply_params(tetra_demod* h, const host::DesignParams& np, bool tables, bool new_tap_count, bool timing_reset) {
    host::Design nd = h->design;          // caller-supplied tables and everything a setter does not own are carried over
    if (!host::params_ok(np)) return TETRA_ERR_UNSUPPORTED;
    if (tables) {
        // A caller-supplied RRC table is the caller's: the rate setters leave it alone and do the rest of their work (timing loop:
        // COMPLEX_FD::setOmega); the caller follows with tetra_demod_set_tables (what the SDR++ build of the C++ mirror does with
        // taps::rootRaisedCosine's output, pi4dqpsk.cpp:36-40).  A setter that ONLY re-designs the RRC has nothing left to do.
        if (h->user_rrc && !timing_reset) return TETRA_ERR_UNSUPPORTED;
        if (!h->user_rrc) host::design_rrc(np, nd);
        if (new_tap_count && !h->quirks && np.rrc_tap_count != nd.ntaps_be) {
            if (h->user_be) return TETRA_ERR_UNSUPPORTED;
            host::design_bandedge(np, nd, np.rrc_tap_count);           // documented deviation: one length for the three FIRs
        }
        if (nd.ntaps > kGenMaxTaps || nd.ntaps_be > kGenMaxTaps) return TETRA_ERR_UNSUPPORTED;   // (params_ok has said so already)
    }
    host::design_loops(np, nd);
    host::design_timing_limits(np, nd);
    if (stride_for(nd, h->max_samples) > 0x7ffffff0ll) return TETRA_ERR_UNSUPPORTED;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    if (h->taps_sym() && stride_for(nd, h->max_samples) / 2 > h->q_sym_stride) {
        // a slower timing loop emits more symbols per sample: the statistic's symbol scratch grows with it
        const long long want = stride_for(nd, h->max_samples) / 2;
        DevMem<float2> q;
        HIP_TRY(h, q.reserve(sizeof(float2) * (size_t)h->C * (size_t)want));
        h->q_sym = std::move(q);
        h->q_sym_stride = want;
    }
    const int old_ntaps = h->design.ntaps;
    int rc = commit_design(h, np, nd);
    if (rc != TETRA_OK) return rc;
    if (tables && ((rc = upload_tables(h)) || (rc = shrink_rrc_valid(h, old_ntaps)))) return rc;
    if (timing_reset) {
        if ((rc = reset_timing(h, 0, h->C))) return rc;
        HIP_TRY(h, hipStreamSynchronize(0));
    }
    return TETRA_OK;
}
}  // namespace

int tetra_demod_set_param(tetra_demod_t* h, int param_id, double value) {
    if (!h) return TETRA_ERR_ARG;
    host::DesignParams np = h->dp;
    bool timing_reset = false, tables = false;
    switch (param_id) {
    // loop setters (pi4dqpsk.cpp:76-118): loop constants only
    case TETRA_PARAM_AGC_RATE: np.agc_rate = value; break;
    case TETRA_PARAM_COSTAS_BANDWIDTH: np.costas_bandwidth = value; break;
    case TETRA_PARAM_FLL_BANDWIDTH: np.fll_bandwidth = value; break;
    case TETRA_PARAM_OMEGA_GAIN: np.omega_gain = value; break;
    case TETRA_PARAM_MU_GAIN: np.mu_gain = value; break;
    case TETRA_PARAM_OMEGA_REL_LIMIT: np.omega_rel_limit = value; break;
    // rate setters (pi4dqpsk.cpp:32-54): RRC taps + COMPLEX_FD::setOmega; the FLL's filters are not touched
    case TETRA_PARAM_SYMBOLRATE:
    case TETRA_PARAM_SAMPLERATE:
        if (param_id == TETRA_PARAM_SYMBOLRATE) np.symbolrate = value; else np.samplerate = value;
        timing_reset = tables = true;
        break;
    // setRRCTapCount / the beta half of setRRCParams (pi4dqpsk.cpp:56-74)
    case TETRA_PARAM_RRC_TAP_COUNT: np.rrc_tap_count = (int)value; tables = true; break;
    case TETRA_PARAM_RRC_BETA: np.rrc_beta = value; tables = true; break;
    default: return TETRA_ERR_ARG;
    }
    return apply_params(h, np, tables, param_id == TETRA_PARAM_RRC_TAP_COUNT, timing_reset);
}

// PI4DQPSK::setRRCParams (pi4dqpsk.cpp:56-66): tap count and roll-off in ONE re-design of the RRC.
int tetra_demod_set_rrc_params(tetra_demod_t* h, int rrc_tap_count, double rrc_beta) {
    if (!h) return TETRA_ERR_ARG;
    host::DesignParams np = h->dp;
    np.rrc_tap_count = rrc_tap_count;
    np.rrc_beta = rrc_beta;
    return apply_params(h, np, true, true, false);
}

// FIR::setTaps with tables the CALLER designed (ABI 5): what PI4DQPSK::init / setSymbolrate / setSamplerate / setRRCParams do with
// the output of SDR++'s own generators (pi4dqpsk.cpp:18-19,38-39,50-51,63-64), FLL::createBandedgeFilters (fll.cpp:61-95) and
// COMPLEX_FD::generateInterpTaps (complex_fd.cpp:153-158).
int tetra_demod_set_tables(tetra_demod_t* h, const float* rrc_taps, int n_rrc, const float* bandedge_taps, int n_be,
                           const float* interp_bank) {
    if (!h) return TETRA_ERR_ARG;
    if (!rrc_taps && !bandedge_taps && !interp_bank) return TETRA_ERR_ARG;
    if (rrc_taps && (n_rrc < 2 || n_rrc > kGenMaxTaps)) return TETRA_ERR_UNSUPPORTED;
    if (bandedge_taps && (n_be < 2 || n_be > kGenMaxTaps)) return TETRA_ERR_UNSUPPORTED;
    host::Design nd = h->design;
    host::DesignParams np = h->dp;
    if (rrc_taps) {
        nd.ntaps = n_rrc;
        nd.rrc.assign(rrc_taps, rrc_taps + n_rrc);
        np.rrc_tap_count = n_rrc;
    }
    if (bandedge_taps) {
        nd.ntaps_be = n_be;
        nd.be_re.assign(bandedge_taps, bandedge_taps + n_be);
        nd.be_im.assign(bandedge_taps + n_be, bandedge_taps + 2 * (size_t)n_be);
    }
    if (interp_bank) nd.bank.assign(interp_bank, interp_bank + kInterpPhases * kInterpTaps);
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    const int old_ntaps = h->design.ntaps;
    // commit, upload -- and take the commit back if the upload fails: the handle never stays half-updated (its host-side design is
    // what the next setter re-designs from and what get_tables reports)
    const host::Design old_design = h->design;
    const host::DesignParams old_dp = h->dp;
    const bool old_user_rrc = h->user_rrc, old_user_be = h->user_be;
    int rc = commit_design(h, np, nd);
    if (rc != TETRA_OK) return rc;
    if (rrc_taps) h->user_rrc = true;
    if (bandedge_taps) h->user_be = true;
    if ((rc = upload_tables(h)) != TETRA_OK) {
        (void)commit_design(h, old_dp, old_design);
        h->user_rrc = old_user_rrc;
        h->user_be = old_user_be;
        (void)upload_tables(h);
        return rc;
    }
    return shrink_rrc_valid(h, old_ntaps);
}

int tetra_demod_get_state(tetra_demod_t* h, int channel, tetra_demod_channel_state_t* out) {
    if (!h || !out || channel < 0 || channel >= h->C) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    const int c = channel;
#define GET1(dst, src) HIP_TRY(h, hipMemcpy(&(dst), (src) + c, sizeof(dst), hipMemcpyDeviceToHost))
    GET1(out->agc_gain, h->agc_g); GET1(out->fll_phase, h->fll_ph); GET1(out->fll_freq, h->fll_fr);
    GET1(out->mu, h->mu); GET1(out->omega, h->omega); GET1(out->offset, h->offset);
    GET1(out->costas_phase, h->cph); GET1(out->costas_freq, h->cfr); GET1(out->ph2, h->ph2); GET1(out->prev, h->prev);
    GET1(out->rrc_valid, h->rrc_valid);
#undef GET1
    HIP_TRY(h, hipMemcpy(out->hist, h->hist + (size_t)c * kHist, sizeof(float2) * kHist, hipMemcpyDeviceToHost));
    if (h->far_valid)
        HIP_TRY(h, hipMemcpy(out->hist_far, h->hist_far + (size_t)c * (kGenHist - kHist), sizeof(float2) * (kGenHist - kHist), hipMemcpyDeviceToHost));
    else
        std::memset(out->hist_far, 0, sizeof(out->hist_far));
    HIP_TRY(h, hipMemcpy(out->ybuf, h->ybuf + (size_t)c * kYHist, sizeof(float2) * kYHist, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

int tetra_demod_set_state(tetra_demod_t* h, int channel, const tetra_demod_channel_state_t* in) {
    if (!h || !in || channel < 0 || channel >= h->C) return TETRA_ERR_ARG;
    // Phases outside what the loops can produce are refused (every pcl.advance wraps to [-pi, pi], ph2 to (-2 pi, 2 pi),
    // pi4dqpsk_costas.cpp:10-15): the kernel's phasor evaluation relies on those ranges.  NaN (a poisoned channel) passes.
    if (std::fabs(in->fll_phase) > kFlPi || std::fabs(in->costas_phase) > kFlPi || std::fabs(in->ph2) >= 2 * kFlPi) return TETRA_ERR_ARG;
    // The carried read position of the timing loop is >= 0 by construction (complex_fd.cpp:141-148: offset -= count only after
    // the loop left with offset >= count) and mu is a fraction in [0, 1) -- or NaN on a poisoned channel; a negative offset or an
    // infinite mu would index the kernels' delay lines out of range.
    if (in->offset < 0 || std::isinf(in->mu)) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    const int c = channel;
#define SET1(dst, src) HIP_TRY(h, hipMemcpy((dst) + c, &(src), sizeof(src), hipMemcpyHostToDevice))
    // a phase of -0 is stored as +0: the loops never produce one (a sum is -0 only for two -0 operands, and the chain starts at
    // +0), and the FLL blocks' rint-based phase wrap (gen_fll_asm.py) would turn it into +0 one step later than the reference
    const float fll_phase = in->fll_phase == 0.0f ? 0.0f : in->fll_phase;
    const float costas_phase = in->costas_phase == 0.0f ? 0.0f : in->costas_phase;      // (the Costas wave wraps the same way)
    SET1(h->agc_g, in->agc_gain); SET1(h->fll_ph, fll_phase); SET1(h->fll_fr, in->fll_freq);
    SET1(h->mu, in->mu); SET1(h->omega, in->omega); SET1(h->offset, in->offset);
    SET1(h->cph, costas_phase); SET1(h->cfr, in->costas_freq); SET1(h->ph2, in->ph2); SET1(h->prev, in->prev);
    const int rv = in->rrc_valid < 0 ? 0 : in->rrc_valid > (int)kGenHist ? (int)kGenHist : in->rrc_valid;
    SET1(h->rrc_valid, rv);
#undef SET1
    HIP_TRY(h, hipMemcpy(h->hist + (size_t)c * kHist, in->hist, sizeof(float2) * kHist, hipMemcpyHostToDevice));
    if (!h->far_valid) {      // the far delay line of EVERY channel reads as zeros right now: make that literal, then this channel's is current
        HIP_TRY(h, hipMemset(h->hist_far, 0, sizeof(float2) * (kGenHist - kHist) * (size_t)h->C));
        h->far_valid = true;
    }
    HIP_TRY(h, hipMemcpy(h->hist_far + (size_t)c * (kGenHist - kHist), in->hist_far, sizeof(float2) * (kGenHist - kHist), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->ybuf + (size_t)c * kYHist, in->ybuf, sizeof(float2) * kYHist, hipMemcpyHostToDevice));
    return TETRA_OK;
}

int tetra_demod_get_tables(tetra_demod_t* h, int* taps, float* rrc, int* be_taps, float* be_re, float* be_im, float* bank) {
    if (!h) return TETRA_ERR_ARG;
    const int nt = h->design.ntaps;
    if (taps) *taps = nt;
    if (be_taps) *be_taps = h->design.ntaps_be;
    if (rrc) std::memcpy(rrc, h->design.rrc.data(), sizeof(float) * nt);
    if (be_re) std::memcpy(be_re, h->design.be_re.data(), sizeof(float) * h->design.ntaps_be);
    if (be_im) std::memcpy(be_im, h->design.be_im.data(), sizeof(float) * h->design.ntaps_be);
    if (bank) std::memcpy(bank, h->design.bank.data(), sizeof(float) * kInterpPhases * kInterpTaps);
    return TETRA_OK;
}

int tetra_demod_bandedge_tap_count(tetra_demod_t* h) { return h ? h->design.ntaps_be : TETRA_ERR_ARG; }

int tetra_demod_debug_read_rrc_out(tetra_demod_t* h, float* y, int n_samples) {
    if (!h || !y || n_samples < 0 || n_samples > h->max_samples) return TETRA_ERR_ARG;
    if (!h->y) return TETRA_ERR_UNSUPPORTED;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    // rows kYHist.. of the time-major scratch hold this call's y
    const size_t C = (size_t)h->C;
    std::vector<float2> tm((size_t)n_samples * C);
    if (n_samples)
        HIP_TRY(h, hipMemcpy(tm.data(), h->y + (size_t)kYHist * C, sizeof(float2) * tm.size(), hipMemcpyDeviceToHost));
    float2* out = reinterpret_cast<float2*>(y);
    for (size_t c = 0; c < C; c++)
        for (size_t i = 0; i < (size_t)n_samples; i++) out[c * (size_t)n_samples + i] = tm[i * C + c];
    return TETRA_OK;
}

int tetra_demod_kernel_ms_history(tetra_demod_t* h, int n, float* ms) {
    if (!h || !ms || n < 1 || n > tetra_demod::kEvSlots || (long long)n > h->n_calls) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    for (int i = 0; i < n; i++) {
        const Event* ev = h->ev[(h->n_calls - n + i) % tetra_demod::kEvSlots];
        HIP_TRY(h, hipEventSynchronize(ev[1]));
        HIP_TRY(h, hipEventElapsedTime(&ms[i], ev[0], ev[1]));
    }
    return TETRA_OK;
}

int tetra_demod_last_kernel_ms(tetra_demod_t* h, float* ms) { return tetra_demod_kernel_ms_history(h, 1, ms); }

int tetra_demod_get_quality(tetra_demod_t* h, float* standarderr, uint8_t* sync) {
    if (!h) return TETRA_ERR_ARG;
    if (!h->q_ring) return TETRA_ERR_UNSUPPORTED;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    if (standarderr) HIP_TRY(h, hipMemcpy(standarderr, h->q_err, sizeof(float) * (size_t)h->C, hipMemcpyDeviceToHost));
    if (sync) {
        std::vector<int> tmp((size_t)h->C);
        HIP_TRY(h, hipMemcpy(tmp.data(), h->q_sync, sizeof(int) * (size_t)h->C, hipMemcpyDeviceToHost));
        for (int c = 0; c < h->C; c++) sync[c] = (uint8_t)(tmp[c] != 0);
    }
    return TETRA_OK;
}

int tetra_demod_get_constellation(tetra_demod_t* h, int first, int count, float* symbols, int32_t* n_blocks) {
    if (!h) return TETRA_ERR_ARG;
    if (!h->cd_blk) return TETRA_ERR_UNSUPPORTED;
    if (first < 0 || count < 0 || first > h->C || count > h->C - first) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    if (count == 0) return TETRA_OK;
    if (symbols)
        HIP_TRY(h, hipMemcpy(symbols, h->cd_blk + (size_t)first * kCdSyms, sizeof(float2) * kCdSyms * (size_t)count, hipMemcpyDeviceToHost));
    if (n_blocks) HIP_TRY(h, hipMemcpy(n_blocks, h->cd_blocks + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

int tetra_demod_last_hip_error(tetra_demod_t* h) { return h ? h->last_hip : 0; }

int tetra_demod_debug_selftest(tetra_demod_t* h, const float* in128, float* out320) {
    if (!h || !in128 || !out320) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    DevMem<float> din, dout;          // freed on every return path
    HIP_TRY(h, din.reserve(sizeof(float) * 128));
    HIP_TRY(h, dout.reserve(sizeof(float) * 320));
    HIP_TRY(h, hipMemcpy(din, in128, sizeof(float) * 128, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_selftest, dim3(1), dim3(64), 0, 0, din, dout);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpy(out320, dout, sizeof(float) * 320, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

int tetra_demod_debug_mfma_selftest(tetra_demod_t* h, int shape, int k, const float* a, const float* b, float* d) {
    if (!h || !a || !b || !d || (shape != 16 && shape != 32) || k < 4 || (k & 3) || k > 4096) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    DevMem<float> da, db, dd;
    const size_t na = (size_t)shape * k, nd = (size_t)shape * shape;
    HIP_TRY(h, da.reserve(sizeof(float) * na));
    HIP_TRY(h, db.reserve(sizeof(float) * na));
    HIP_TRY(h, dd.reserve(sizeof(float) * nd));
    HIP_TRY(h, hipMemcpy(da, a, sizeof(float) * na, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(db, b, sizeof(float) * na, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_mfma_selftest, dim3(1), dim3(64), 0, 0, shape, k, da, db, dd);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpy(d, dd, sizeof(float) * nd, hipMemcpyDeviceToHost));
    return TETRA_OK;
}

}  // extern "C"
