// tetra_resamp.hip -- rational resampler on time-major frames (include/tetra_chan.h, round 6): HIP kernels + C ABI.
//
// Sits between the channeliser (50 ksps per channel) and the demodulator, which then runs at the reference instance's own rate:
// VFO_SAMPLERATE 36000, 2 samples per symbol (/root/reference/src/main.cpp:35,75,84).  Bound by its HBM traffic: per input frame of C
// channels 8 C bytes are read and 8 C I / DN written (config 5, a quarter second: 80 MB + 57.6 MB); the arithmetic (2 T flop per
// output float) is a tenth of what the vector pipes do in that time.  Thread-level code: resamp_core.hpp.
// Picked columns may carry an offset each (include/ext/tetra_carrier_offset.h): the mixing kernels (Cols = resamp::MixColumns) are
// launched only while some offset is non-zero; without one the launches are the ones of a handle that knows no offsets.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/tetra_chan.h"
#include "chan_design.hpp"
#include "hip_host.hpp"
#include "resamp_core.hpp"
#include "resamp_handle.hpp"
#include "retune_impl.hpp"

namespace {

constexpr int kThreads = 256;

// Workgroups are dealt to the 8 XCDs round-robin (each XCD has its own L2) and consecutive groups share T - 1 of their DN + T - 1
// rows: the XCD a workgroup lands on (blockIdx.x mod 8) takes a CONTIGUOUS range of the launch's thread blocks, so that a row's
// second reader finds it in the L2 its first reader filled.
__device__ __forceinline__ long long remapped_block(int span) {
    return (long long)(blockIdx.x & 7) * span + (long long)(blockIdx.x >> 3);
}

// The two kernels, over every column in place (no Cols: resamp::AllColumns) or over picked columns (Cols = resamp::PickColumns, the
// wideband receiver's carriers: one channel per lane unit, read from column cols.col[u] of the channeliser's rows).  The column map
// keeps the place it has had in the argument list, so both forms keep their kernarg layout; Cols is always named, never deduced.
template <int I, int DN, int T, int W, class... Cols> __global__ __launch_bounds__(kThreads) void k_resample(resamp::Ctx c, Cols... cols, int span, long long blocks) {
    const long long b = remapped_block(span);
    if (b >= blocks) return;
    resamp::thread_fixed<I, DN, T, W>(c, b * kThreads + threadIdx.x, cols...);
}

template <int W, class... Cols> __global__ __launch_bounds__(kThreads) void k_resample_generic(resamp::Ctx c, Cols... cols, int span, long long blocks) {
    const long long b = remapped_block(span);
    if (b >= blocks) return;
    resamp::thread_generic<W>(c, b * kThreads + threadIdx.x, cols...);
}

// rows [first, first + rows) of frames [*][in_ch], columns cols[0 .. n) -> out [rows][n] (the picked delay line)
__global__ __launch_bounds__(256) void k_pick_rows(const float2* __restrict__ in, int in_ch, const int32_t* __restrict__ cols, int n,
                                                   long long first, int rows, float2* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)rows * n) return;
    const long long r = i / n;
    const int j = (int)(i - r * n);
    out[i] = in[(first + r) * in_ch + cols[j]];
}

// the kernels of a ratio in resamp_core.hpp's table, nullptr for any other
fixed_kernel_t pick_fixed(int I, int DN, int T, int W) {
    fixed_kernel_t k = nullptr;
    resamp::visit_ratio(I, DN, T, [&](auto r) {
        using R = decltype(r);
        k = W == 4 ? (fixed_kernel_t)k_resample<R::I, R::DN, R::T, 4> : (fixed_kernel_t)k_resample<R::I, R::DN, R::T, 2>;
    });
    return k;
}
pick_kernel_t pick_picked(int I, int DN, int T) {
    pick_kernel_t k = nullptr;
    resamp::visit_ratio(I, DN, T, [&](auto r) {
        using R = decltype(r);
        k = (pick_kernel_t)k_resample<R::I, R::DN, R::T, 2, resamp::PickColumns>;
    });
    return k;
}
mix_kernel_t pick_mixed(int I, int DN, int T) {
    mix_kernel_t k = nullptr;
    resamp::visit_ratio(I, DN, T, [&](auto r) {
        using R = decltype(r);
        k = (mix_kernel_t)k_resample<R::I, R::DN, R::T, 2, resamp::MixColumns>;
    });
    return k;
}

// Kaiser-windowed sinc at the zero-stuffed rate, cutoff fc = cutoff_rel / (2 max(I, DN)) cycles per sample there (= cutoff_rel x the
// narrower of the input and output Nyquist bands), DC gain I.
void design_prototype(int I, int DN, int T, double cutoff_rel, double beta, std::vector<float>& h) {
    chandesign::kaiser_sinc(I * T, cutoff_rel / (2.0 * (double)(I > DN ? I : DN)), beta, (double)I, h);
}

}  // namespace


namespace {

// One call's kernel and delay-line carry.  d_cols = nullptr: every column in place (in_ch = C); else the C picked columns of rows of
// in_ch channels.  The arguments are checked by the caller.
int process_any(tetra_resamp* h, const int32_t* d_cols, int in_ch, const float* d_in, int n_in, float* d_out, int* n_out, hipStream_t s) {
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    const long long m1 = resamp::outputs_after(h->n_total + n_in, h->I, h->DN);
    const long long n_new = m1 - h->m_next;
    *n_out = (int)n_new;
    HIP_TRY(h, hipEventRecord(h->ev[0], s));
    if (n_new > 0) {
        resamp::Ctx c;
        c.x = d_in; c.hist = h->hist; c.out = d_out; c.coef = h->d_coef;
        c.n0 = h->n_total; c.m0 = h->m_next; c.m1 = m1; c.n_in = n_in; c.units = h->units;
        c.I = h->I; c.DN = h->DN; c.T = h->T;
        long long threads;
        if (d_cols ? h->pick != nullptr : h->fixed != nullptr) threads = ((m1 + h->I - 1) / h->I - h->m_next / h->I) * (long long)h->units;
        else threads = n_new * (long long)h->units;
        const long long blocks = (threads + kThreads - 1) / kThreads;
        const int span = (int)((blocks + 7) / 8);
        if (d_cols && h->mixing) {
            resamp::MixColumns cols;
            cols.col = d_cols; cols.in_units = in_ch;
            cols.step = reinterpret_cast<const resamp::f2*>(h->d_mix.get());
            cols.inc = h->d_mix.get() + resamp_impl::mix_words(h) - (size_t)h->C;
            if (h->pick_mix) hipLaunchKernelGGL(h->pick_mix, dim3(8 * span), dim3(kThreads), 0, s, c, cols, span, blocks);
            else hipLaunchKernelGGL((k_resample_generic<2, resamp::MixColumns>), dim3(8 * span), dim3(kThreads), 0, s, c, cols, span, blocks);
        } else if (d_cols) {
            resamp::PickColumns cols;
            cols.col = d_cols; cols.in_units = in_ch;
            if (h->pick) hipLaunchKernelGGL(h->pick, dim3(8 * span), dim3(kThreads), 0, s, c, cols, span, blocks);
            else hipLaunchKernelGGL((k_resample_generic<2, resamp::PickColumns>), dim3(8 * span), dim3(kThreads), 0, s, c, cols, span, blocks);
        } else if (h->fixed) hipLaunchKernelGGL(h->fixed, dim3(8 * span), dim3(kThreads), 0, s, c, span, blocks);
        else if (h->W == 4) hipLaunchKernelGGL(k_resample_generic<4>, dim3(8 * span), dim3(kThreads), 0, s, c, span, blocks);
        else hipLaunchKernelGGL(k_resample_generic<2>, dim3(8 * span), dim3(kThreads), 0, s, c, span, blocks);
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(h->ev[1], s));
    h->ev_valid = true;
    // carry (DelayLine): the newest frames' rows as they are, or their picked columns
    const size_t row = 2 * (size_t)h->C;
    HIP_TRY(h, h->hist.carry((size_t)n_in, s, [&](float* dst, size_t from_x) {
        if (!d_cols) return hipMemcpyAsync(dst, d_in + row * ((size_t)n_in - from_x), sizeof(float) * row * from_x, hipMemcpyDeviceToDevice, s);
        const long long n = (long long)from_x * h->C;
        hipLaunchKernelGGL(k_pick_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float2*>(d_in), in_ch, d_cols, h->C,
                           (long long)n_in - (long long)from_x, (int)from_x, reinterpret_cast<float2*>(dst));
        return hipGetLastError();
    }));
    h->n_total += n_in;
    h->m_next = m1;
    return TETRA_OK;
}

}  // namespace

namespace resamp_impl {

int process_pick_device(tetra_resamp_t* h, const int32_t* d_cols, int in_ch, const float* d_in, int n_in, float* d_out, int* n_out, hipStream_t s) {
    if (!h || !d_cols || in_ch < 1 || (!d_in && n_in > 0) || !d_out || !n_out || h->W != 2) return TETRA_ERR_ARG;
    if (n_in < 0 || n_in > h->max_in) return TETRA_ERR_SIZE;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return TETRA_ERR_ALIGN;
    return process_any(h, d_cols, in_ch, d_in, n_in, d_out, n_out, s);
}

size_t mix_words(const tetra_resamp_t* h) { return (size_t)h->C * (1 + 2 * (size_t)resamp::mix_rows(h->I, h->DN, h->T)); }

void mix_fill(const tetra_resamp_t* h, const uint32_t* inc, int32_t* words) {
    const int rows = resamp::mix_rows(h->I, h->DN, h->T);
    resamp::step_table(inc, h->C, rows, reinterpret_cast<float*>(words));
    std::memcpy(words + 2 * (size_t)rows * h->C, inc, sizeof(uint32_t) * (size_t)h->C);
}

int set_mix(tetra_resamp_t* h, const uint32_t* inc, const int32_t* d_tables, hipStream_t s) {
    if (!h || !inc || h->W != 2) return TETRA_ERR_ARG;
    bool any = false;
    for (int j = 0; j < h->C; j++) any = any || inc[j] != 0;
    if (any && !d_tables) return TETRA_ERR_ARG;
    if (d_tables) {
        DeviceGuard g(h->device);
        if (!g.ok) return TETRA_ERR_NO_DEVICE;
        const size_t bytes = sizeof(int32_t) * mix_words(h);
        HIP_TRY(h, h->d_mix.reserve(bytes));      // (one size for the handle's life: never grown while a kernel reads it)
        HIP_TRY(h, hipMemcpyAsync(h->d_mix, d_tables, bytes, hipMemcpyDeviceToDevice, s));
    }
    h->inc.assign(inc, inc + h->C);
    h->mixing = any;
    return TETRA_OK;
}

}  // namespace resamp_impl

int retune_impl::resamp_narrow_units(tetra_resamp_t* h) {
    if (!h) return TETRA_ERR_ARG;
    h->W = 2;
    h->units = h->C;
    h->fixed = (h->cfg.flags & TETRA_RESAMP_FLAG_GENERIC) ? nullptr : pick_fixed(h->I, h->DN, h->T, h->W);
    h->cfg.flags |= TETRA_RESAMP_FLAG_NARROW_UNITS;
    return TETRA_OK;
}

extern "C" {

int tetra_resamp_default_config(tetra_resamp_config_t* cfg) {
    if (!cfg) return TETRA_ERR_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_channels = 800;
    cfg->interp = 18;
    cfg->decim = 25;
    cfg->taps_per_phase = 16;
    cfg->max_in = 1 << 16;
    cfg->device = -1;
    cfg->cutoff_rel = 1.0;
    cfg->kaiser_beta = 6.0;
    return TETRA_OK;
}

int tetra_resamp_create(const tetra_resamp_config_t* cfg, tetra_resamp_t** out) {
    if (!cfg || !out) return TETRA_ERR_ARG;
    *out = nullptr;
    if (cfg->n_channels < 1 || cfg->interp < 1 || cfg->decim < 1 || cfg->taps_per_phase < 2 || cfg->taps_per_phase > 64 ||
        cfg->interp > 4096 || cfg->decim > 4096 || cfg->max_in < 1 || cfg->reserved != 0 ||
        (cfg->flags & ~(TETRA_RESAMP_FLAG_GENERIC | TETRA_RESAMP_FLAG_NARROW_UNITS)) || !(cfg->cutoff_rel > 0) || !(cfg->kaiser_beta >= 0))
        return TETRA_ERR_ARG;
    // the outputs of one call are addressed with 32-bit frame counts
    if ((long long)cfg->max_in * cfg->interp / cfg->decim + 2 > 0x7fffffffLL) return TETRA_ERR_SIZE;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return TETRA_ERR_NO_DEVICE;
    if (dev >= ndev) return TETRA_ERR_NO_DEVICE;
    tetra_resamp* h = new (std::nothrow) tetra_resamp();
    if (!h) return TETRA_ERR_NOMEM;
    h->cfg = *cfg;
    h->cfg.prototype = nullptr;
    h->device = dev;
    h->C = cfg->n_channels; h->I = cfg->interp; h->DN = cfg->decim; h->T = cfg->taps_per_phase; h->max_in = cfg->max_in;
    h->W = (h->C % 2 == 0 && !(cfg->flags & TETRA_RESAMP_FLAG_NARROW_UNITS)) ? 4 : 2;                     // 16-byte lane units when a row divides into them
    h->units = 2 * h->C / h->W;
    if (cfg->prototype) h->proto.assign(cfg->prototype, cfg->prototype + (size_t)h->I * h->T);
    else design_prototype(h->I, h->DN, h->T, cfg->cutoff_rel, cfg->kaiser_beta, h->proto);
    h->fixed = (cfg->flags & TETRA_RESAMP_FLAG_GENERIC) ? nullptr : pick_fixed(h->I, h->DN, h->T, h->W);
    h->pick = (cfg->flags & TETRA_RESAMP_FLAG_GENERIC) ? nullptr : pick_picked(h->I, h->DN, h->T);
    h->pick_mix = (cfg->flags & TETRA_RESAMP_FLAG_GENERIC) ? nullptr : pick_mixed(h->I, h->DN, h->T);
    DeviceGuard g(dev);
    if (!g.ok) { delete h; return TETRA_ERR_NO_DEVICE; }
    std::vector<float> coef((size_t)h->I * h->T);
    if (h->fixed) resamp::phase_table(h->proto.data(), h->I, h->DN, h->T, coef.data());
    else coef = h->proto;
    bool ok = h->d_coef.reserve(sizeof(float) * coef.size()) == hipSuccess &&
              h->hist.reserve((size_t)h->T - 1, 2 * (size_t)h->C) == hipSuccess &&
              hipEventCreate(h->ev[0].put()) == hipSuccess && hipEventCreate(h->ev[1].put()) == hipSuccess;
    int rc = ok ? TETRA_OK : TETRA_ERR_NOMEM;
    if (rc == TETRA_OK && (hipMemcpy(h->d_coef, coef.data(), sizeof(float) * coef.size(), hipMemcpyHostToDevice) != hipSuccess ||
                           h->hist.reset() != hipSuccess))
        rc = TETRA_ERR_HIP;
    if (rc != TETRA_OK) { delete h; return rc; }
    *out = h;
    return TETRA_OK;
}

int tetra_resamp_destroy(tetra_resamp_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return TETRA_OK;
}

int tetra_resamp_frames_for(tetra_resamp_t* h, int n_in) {
    if (!h || n_in < 0) return TETRA_ERR_ARG;
    return (int)(resamp::outputs_after(h->n_total + n_in, h->I, h->DN) - h->m_next);
}

int tetra_resamp_process_device(tetra_resamp_t* h, const float* d_in, int n_in, float* d_out, int* n_out, void* hip_stream) {
    if (!h || (!d_in && n_in > 0) || !d_out || !n_out) return TETRA_ERR_ARG;
    if (n_in < 0 || n_in > h->max_in) return TETRA_ERR_SIZE;
    const size_t amask = h->W == 4 ? 15 : 7;
    if (((uintptr_t)d_in & amask) || ((uintptr_t)d_out & amask)) return TETRA_ERR_ALIGN;
    return process_any(h, nullptr, h->C, d_in, n_in, d_out, n_out, (hipStream_t)hip_stream);
}

int tetra_resamp_process(tetra_resamp_t* h, const float* in, int n_in, float* out, int* n_out) {
    if (!h || (!in && n_in > 0) || !out || !n_out) return TETRA_ERR_ARG;
    if (n_in < 0 || n_in > h->max_in) return TETRA_ERR_SIZE;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    const size_t row = sizeof(float) * 2 * (size_t)h->C;
    const size_t frames = (size_t)(resamp::outputs_after(h->n_total + n_in, h->I, h->DN) - h->m_next);
    HIP_TRY(h, h->st_in.reserve(row * (n_in ? (size_t)n_in : 1)));
    HIP_TRY(h, h->st_out.reserve(row * (frames ? frames : 1)));
    if (n_in > 0) HIP_TRY(h, hipMemcpy(h->st_in, in, row * (size_t)n_in, hipMemcpyHostToDevice));
    int rc = tetra_resamp_process_device(h, h->st_in, n_in, h->st_out, n_out, nullptr);
    if (rc == TETRA_OK) {
        hipError_t e = hipStreamSynchronize(0);
        if (e == hipSuccess && frames) e = hipMemcpy(out, h->st_out, row * frames, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { h->last_hip = (int)e; rc = TETRA_ERR_HIP; }
    }
    return rc;
}

int tetra_resamp_reset(tetra_resamp_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->hist.reset());
    h->n_total = 0;
    h->m_next = 0;
    return TETRA_OK;
}

int tetra_resamp_get_prototype(tetra_resamp_t* h, float* proto) {
    if (!h || !proto) return TETRA_ERR_ARG;
    std::memcpy(proto, h->proto.data(), sizeof(float) * h->proto.size());
    return TETRA_OK;
}

int tetra_resamp_last_kernel_ms(tetra_resamp_t* h, float* ms) {
    if (!h || !ms || !h->ev_valid) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipEventSynchronize(h->ev[1]));
    HIP_TRY(h, hipEventElapsedTime(ms, h->ev[0], h->ev[1]));
    return TETRA_OK;
}

}  // extern "C"
