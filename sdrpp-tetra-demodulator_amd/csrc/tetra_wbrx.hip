// tetra_wbrx.hip -- the wideband receiver behind one handle (include/tetra_wbrx.h): one capture in, the receive chain's blocks per
// carrier out.  Per call k, all on the caller's stream:
//
//   [wait: call k - 1 is through]  channeliser (tetra_chan) -> chan_out [nf][M]                                   (event C_k)
//                                  selecting resampler: the carriers' columns of chan_out -> res[k & 1] [n][n_bins]  (event R_k)
//                                  tetra_rx_process_device(res[k & 1], n): demodulator here, the chain's tail on its own stream
//
// The resampler's state (delay line of the picked columns, positions) is a tetra_resamp handle created for n_bins channels with
// one channel per lane unit; resamp_impl::process_pick_device runs its kernels over picked columns (resamp_core.hpp, PickColumns).
// A bin list 0 .. M - 1 in order runs the resampler in place on the full rows instead.  The resampled frames are double buffered by
// call parity like the chain's bit rows, so tetra_wbrx_frames_device can hand out the previous call's too.
//
// Per-carrier offsets (include/ext/tetra_carrier_offset.h) are the selecting resampler's: with a non-zero one in force it rotates each
// carrier's column as it loads it (resamp_core.hpp, MixColumns).  chan_out, the delay line and the retune ring stay un-rotated.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../../include/ext/tetra_carrier_offset.h"
#include "../../include/ext/tetra_gap.h"
#include "../../include/ext/tetra_iqcond.h"
#include "../../include/tetra_shift.h"
#include "hip_host.hpp"
#include "resamp_handle.hpp"
#include "retune_core.hpp"
#include "retune_impl.hpp"
#include "rx_handle.hpp"
#include "wbrx_handle.hpp"

namespace {

constexpr int kPowerSplits = 4096;      // at most this many frame ranges per bin in the first pass of the bin power
constexpr int kPowerMinFrames = 64;     // and at least this many frames in each

// Partial sums of |X_k|^2 over frames [y F, y F + F) of x [nf][M]: one lane per bin (a row's reads are coalesced), float64 sums.
__global__ __launch_bounds__(256) void k_bin_power_part(const float2* __restrict__ x, int M, int nf, int F, double* __restrict__ part) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    const int f0 = blockIdx.y * F, f1 = f0 + F < nf ? f0 + F : nf;
    double s = 0.0;
    for (int f = f0; f < f1; f++) {
        const float2 v = x[(size_t)f * M + k];
        s += (double)v.x * v.x + (double)v.y * v.y;
    }
    part[(size_t)blockIdx.y * M + k] = s;
}

// out[k] = (sum of the partial sums of bin k) / nf
__global__ __launch_bounds__(256) void k_bin_power_sum(const double* __restrict__ part, int M, int splits, int nf, float* __restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= M) return;
    double s = 0.0;
    for (int j = 0; j < splits; j++) s += part[(size_t)j * M + k];
    out[k] = (float)(s / (double)nf);
}

// The `rows` newest of the n_in frames x [n_in][M] that follow n0 earlier ones -> the history ring (retune_core.hpp)
__global__ __launch_bounds__(256) void k_keep_rows(const float* __restrict__ x, int M, long long n0, int n_in, int rows, int hist, float* __restrict__ ring) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long long)rows * M) retune::keep_element(x, M, n0, n_in, rows, hist, i, ring);
}

bool no_device() {
    int n = 0;
    return hipGetDeviceCount(&n) != hipSuccess || n <= 0;
}

template <typename T> bool dalloc(DevMem<T>& p, size_t count) { return p.reserve(sizeof(T) * (count ? count : 1)) == hipSuccess; }

enum { kFmtC32 = 0, kFmtCs16 = 1, kFmtCs8 = 2 };
constexpr size_t kFmtBytes[3] = { 8, 4, 2 };

int process_any(tetra_wbrx* h, int fmt, const void* d_x, int n_in, void* hip_stream) {
    if (!h || (!d_x && n_in > 0)) return TETRA_ERR_ARG;
    if (n_in < 0 || n_in > h->max_in) return TETRA_ERR_SIZE;
    if ((uintptr_t)d_x & (kFmtBytes[fmt] - 1)) return TETRA_ERR_ALIGN;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int b = (int)(h->calls & 1);
    // chan_out was read by the previous call's resampler and res[b] by the demodulator two calls back (which the previous call
    // waited for in turn): on another stream, wait for them
    if (h->done_recorded) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_done, 0));      // (a retune records it too)
    int nf = 0, nr = 0;
    if (fmt == kFmtCs16) TETRA_TRY(tetra_chan_process_device_cs16(h->chan, static_cast<const int16_t*>(d_x), n_in, h->chan_out, &nf, s));
    else if (fmt == kFmtCs8) TETRA_TRY(tetra_chan_process_device_cs8(h->chan, static_cast<const int8_t*>(d_x), n_in, h->chan_out, &nf, s));
    else TETRA_TRY(tetra_chan_process_device(h->chan, static_cast<const float*>(d_x), n_in, h->chan_out, &nf, s));
    HIP_TRY(h, hipEventRecord(h->ev_chan, s));
    if (h->all) TETRA_TRY(tetra_resamp_process_device(h->rs, h->chan_out, nf, h->res[b], &nr, s));
    else TETRA_TRY(resamp_impl::process_pick_device(h->rs, h->d_bins, h->M, h->chan_out, nf, h->res[b], &nr, s));
    HIP_TRY(h, hipEventRecord(h->ev_res[b], s));
    h->n_chan = nf;
    h->n_res[b] = nr;
    h->calls++;
    TETRA_TRY(tetra_rx_process_device(h->rx, h->res[b], nr, s));
    if (nf > 0) {      // the newest T - 1 channeliser frames of ALL bins, for the slots a retune moves (tetra_retune.hip); off the chain's path
        const tetra_resamp* rs = h->rs;
        const int hist = rs->T - 1, rows = nf < hist ? nf : hist;
        const long long n = (long long)rows * h->M;
        hipLaunchKernelGGL(k_keep_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, h->chan_out.get(), h->M, rs->n_total - nf, nf, rows, hist,
                           h->ring.get());
        HIP_TRY(h, hipGetLastError());
    }
    HIP_TRY(h, hipEventRecord(h->ev_done, s));
    h->done_recorded = true;
    return TETRA_OK;
}

int process_host(tetra_wbrx* h, int fmt, const void* x, int n_in) {
    if (!h || (!x && n_in > 0)) return TETRA_ERR_ARG;
    if (n_in < 0 || n_in > h->max_in) return TETRA_ERR_SIZE;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    if (h->st_x.reserve(kFmtBytes[fmt] * (size_t)h->max_in) != hipSuccess) return TETRA_ERR_NOMEM;
    // the staging buffer is read by the previous call's channeliser (and its delay-line copy): wait for it before overwriting
    HIP_TRY(h, hipStreamSynchronize(nullptr));
    if (n_in > 0) HIP_TRY(h, hipMemcpy(h->st_x, x, kFmtBytes[fmt] * (size_t)n_in, hipMemcpyHostToDevice));
    return process_any(h, fmt, h->st_x, n_in, nullptr);
}

}  // namespace

extern "C" {

int tetra_wbrx_default_config(tetra_wbrx_config_t* cfg) {
    if (!cfg) return TETRA_ERR_ARG;
    std::memset(cfg, 0, sizeof(*cfg));
    TETRA_TRY(tetra_chan_default_config(&cfg->chan));
    tetra_resamp_config_t rc;
    TETRA_TRY(tetra_resamp_default_config(&rc));
    cfg->interp = rc.interp;
    cfg->decim = rc.decim;
    cfg->taps_per_phase = rc.taps_per_phase;
    cfg->resamp_cutoff_rel = rc.cutoff_rel;
    cfg->resamp_kaiser_beta = rc.kaiser_beta;
    TETRA_TRY(tetra_rx_default_config(&cfg->rx));
    cfg->rx.demod.n_channels = 0;             // filled in by the handle
    cfg->rx.demod.max_samples = 0;
    cfg->rx.demod.layout = TETRA_LAYOUT_TIME_MAJOR;
    return TETRA_OK;
}

int tetra_wbrx_create(const tetra_wbrx_config_t* cfg, tetra_wbrx_t** out) {
    if (!cfg || !out) return TETRA_ERR_ARG;
    *out = nullptr;
    const int M = cfg->chan.n_channels, D = cfg->chan.decimation, nb = cfg->n_bins;
    if (M < 1 || D < 1 || cfg->chan.max_in < 1 || nb < 1 || nb > M || !cfg->bins || cfg->interp < 1 || cfg->decim < 1) return TETRA_ERR_ARG;
    std::vector<char> seen((size_t)M, 0);
    for (int j = 0; j < nb; j++) {
        const int k = cfg->bins[j];
        if (k < 0 || k >= M || seen[(size_t)k]) return TETRA_ERR_ARG;
        seen[(size_t)k] = 1;
    }
    // the most frames one call can bring: channeliser (its sub-frame phase carries up to D - 1 samples), then the resampler
    const long long max_chan = ((long long)D - 1 + cfg->chan.max_in) / D;
    const long long max_res = max_chan * cfg->interp / cfg->decim + 1;
    if (max_res > 0x7fffffffLL) return TETRA_ERR_SIZE;
    const tetra_demod_config_t& dc = cfg->rx.demod;
    if ((dc.n_channels != 0 && dc.n_channels != nb) || (dc.layout != 0 && dc.layout != TETRA_LAYOUT_TIME_MAJOR) ||
        (dc.max_samples != 0 && dc.max_samples != (int32_t)max_res))
        return TETRA_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TETRA_ERR_NO_DEVICE;
    int dev = cfg->chan.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return TETRA_ERR_NO_DEVICE;
    if (dev >= ndev) return TETRA_ERR_NO_DEVICE;
    if (dc.device >= 0 && dc.device != dev) return TETRA_ERR_ARG;
    std::unique_ptr<tetra_wbrx> h(new (std::nothrow) tetra_wbrx());      // everything it holds is released on every failure below
    if (!h) return TETRA_ERR_NOMEM;
    h->cfg = *cfg;
    h->bins.assign(cfg->bins, cfg->bins + nb);
    h->cfg.bins = nullptr;
    h->cfg.chan.prototype = nullptr;
    h->device = dev;
    h->M = M; h->n_bins = nb; h->max_in = cfg->chan.max_in; h->max_chan = (int)max_chan; h->max_res = (int)max_res;
    h->all = nb == M;
    for (int j = 0; j < nb && h->all; j++) h->all = h->bins[(size_t)j] == j;
    DeviceGuard g(dev);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;

    tetra_chan_config_t cc = cfg->chan;
    cc.device = dev;
    TETRA_TRY(tetra_chan_create(&cc, h->chan.put()));
    tetra_resamp_config_t rc;
    TETRA_TRY(tetra_resamp_default_config(&rc));
    rc.n_channels = h->all ? M : nb;
    rc.interp = cfg->interp; rc.decim = cfg->decim; rc.taps_per_phase = cfg->taps_per_phase;
    rc.max_in = h->max_chan > 0 ? h->max_chan : 1;
    rc.device = dev;
    rc.flags = h->all ? 0 : TETRA_RESAMP_FLAG_NARROW_UNITS;          // picked columns: one channel per lane unit
    rc.cutoff_rel = cfg->resamp_cutoff_rel; rc.kaiser_beta = cfg->resamp_kaiser_beta;
    TETRA_TRY(tetra_resamp_create(&rc, h->rs.put()));
    tetra_rx_config_t xc = cfg->rx;
    xc.demod.n_channels = nb;
    xc.demod.layout = TETRA_LAYOUT_TIME_MAJOR;
    xc.demod.max_samples = h->max_res;
    xc.demod.device = dev;
    TETRA_TRY(tetra_rx_create(&xc, h->rx.put()));
    static_cast<tetra_rx*>(h->rx)->owned = true;

    const size_t row = 2 * (size_t)nb;
    bool ok = dalloc(h->d_bins, (size_t)nb) && dalloc(h->chan_out, 2 * (size_t)M * (size_t)h->max_chan) &&
              dalloc(h->ring, 2 * (size_t)M * (size_t)(cfg->taps_per_phase - 1)) &&
              dalloc(h->res[0], row * (size_t)h->max_res) && dalloc(h->res[1], row * (size_t)h->max_res) &&
              hipEventCreateWithFlags(h->ev_chan.put(), hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(h->ev_res[0].put(), hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(h->ev_res[1].put(), hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(h->ev_done.put(), hipEventDisableTiming) == hipSuccess;
    if (!ok) return TETRA_ERR_NOMEM;
    HIP_TRY(h.get(), hipMemcpy(h->d_bins, h->bins.data(), sizeof(int32_t) * (size_t)nb, hipMemcpyHostToDevice));
    *out = h.release();
    return TETRA_OK;
}

int tetra_wbrx_destroy(tetra_wbrx_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    (void)hipDeviceSynchronize();
    delete h;
    return TETRA_OK;
}

int tetra_wbrx_reset(tetra_wbrx_t* h) {
    if (!h) return TETRA_ERR_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipDeviceSynchronize());
    TETRA_TRY(tetra_chan_reset(h->chan));
    TETRA_TRY(tetra_resamp_reset(h->rs));
    TETRA_TRY(tetra_rx_reset(h->rx));
    h->calls = 0;
    h->n_chan = 0;
    h->n_res[0] = h->n_res[1] = 0;
    h->at_origin = false;
    return TETRA_OK;
}

int tetra_wbrx_process_device(tetra_wbrx_t* h, const float* d_x, int n_in, void* hip_stream) {
    return process_any(h, kFmtC32, d_x, n_in, hip_stream);
}
int tetra_wbrx_process_device_cs16(tetra_wbrx_t* h, const int16_t* d_x, int n_in, void* hip_stream) {
    return process_any(h, kFmtCs16, d_x, n_in, hip_stream);
}
int tetra_wbrx_process_device_cs8(tetra_wbrx_t* h, const int8_t* d_x, int n_in, void* hip_stream) {
    return process_any(h, kFmtCs8, d_x, n_in, hip_stream);
}
// The process call for a buffer with the driver's sample index (include/ext/tetra_gap.h): a jump forward is a gap, reported to
// tetra_wbrx_gap ahead of the call; everything either of the two refuses is refused here, before anything is enqueued.
int tetra_wbrx_process_device_at(tetra_wbrx_t* h, const void* d_x, int fmt, int n_in, int64_t first_index, const tetra_handover_params_t* p,
                                 void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    static_assert(kFmtC32 == TETRA_IQ_FMT_C64 && kFmtCs16 == TETRA_IQ_FMT_CS16 && kFmtCs8 == TETRA_IQ_FMT_CS8, "process_any's formats are the header's");
    if (!h || fmt < 0 || fmt > kFmtCs8 || (!d_x && n_in > 0)) return TETRA_ERR_ARG;
    if (n_in < 0 || n_in > h->max_in) return TETRA_ERR_SIZE;
    if ((uintptr_t)d_x & (kFmtBytes[fmt] - 1)) return TETRA_ERR_ALIGN;
    if (h->at_origin && first_index < h->at_next) return TETRA_ERR_ARG;          // an overlap
    if (h->at_origin && first_index > h->at_next) TETRA_TRY(tetra_wbrx_gap(h, first_index - h->at_next, p, nullptr, hip_stream));
    h->at_origin = true;
    h->at_next = first_index;          // (a gap has been taken: a process call that fails behind it does not take it twice)
    TETRA_TRY(process_any(h, fmt, d_x, n_in, hip_stream));
    h->at_next = first_index + n_in;
    return TETRA_OK;
}

int tetra_wbrx_process(tetra_wbrx_t* h, const float* x, int n_in) { return process_host(h, kFmtC32, x, n_in); }
int tetra_wbrx_process_cs16(tetra_wbrx_t* h, const int16_t* x, int n_in) { return process_host(h, kFmtCs16, x, n_in); }

tetra_rx_t* tetra_wbrx_rx(tetra_wbrx_t* h) { return h ? (tetra_rx_t*)h->rx : nullptr; }

int tetra_wbrx_bins(tetra_wbrx_t* h, int32_t* out) {
    if (!h || !out) return TETRA_ERR_ARG;
    std::memcpy(out, h->bins.data(), sizeof(int32_t) * h->bins.size());
    return TETRA_OK;
}

int tetra_wbrx_frames_device(tetra_wbrx_t* h, int which, const float** d_frames, int* n_frames, void* hip_stream) {
    if (!h || !d_frames || !n_frames || which < 0 || which > 1) return TETRA_ERR_ARG;
    *d_frames = nullptr;
    *n_frames = 0;
    if (h->calls <= which) return TETRA_OK;
    const int b = (int)((h->calls - 1 - which) & 1);
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    HIP_TRY(h, hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), h->ev_res[b], 0));
    *d_frames = h->res[b];
    *n_frames = h->n_res[b];
    return TETRA_OK;
}

int tetra_wbrx_bin_power(tetra_wbrx_t* h, float* out) {
    if (!h || !out) return TETRA_ERR_ARG;
    const int nf = h->calls > 0 ? h->n_chan : 0, M = h->M;
    if (nf == 0) {
        std::memset(out, 0, sizeof(float) * (size_t)M);
        return TETRA_OK;
    }
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    int F = (nf + kPowerSplits - 1) / kPowerSplits;
    if (F < kPowerMinFrames) F = kPowerMinFrames;
    const int splits = (nf + F - 1) / F;
    if (!h->aux) HIP_TRY(h, hipStreamCreateWithFlags(h->aux.put(), hipStreamNonBlocking));
    HIP_TRY(h, h->pw_part.reserve(sizeof(double) * (size_t)splits * (size_t)M));
    HIP_TRY(h, h->pw_out.reserve(sizeof(float) * (size_t)M));
    HIP_TRY(h, hipStreamWaitEvent(h->aux, h->ev_chan, 0));
    const unsigned gx = (unsigned)((M + 255) / 256);
    hipLaunchKernelGGL(k_bin_power_part, dim3(gx, (unsigned)splits), dim3(256), 0, h->aux, reinterpret_cast<const float2*>(h->chan_out.get()), M,
                       nf, F, h->pw_part);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_bin_power_sum, dim3(gx), dim3(256), 0, h->aux, h->pw_part, M, splits, nf, h->pw_out);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipMemcpyAsync(out, h->pw_out, sizeof(float) * (size_t)M, hipMemcpyDeviceToHost, h->aux));
    HIP_TRY(h, hipStreamSynchronize(h->aux));
    return TETRA_OK;
}

// The frequency shift (include/tetra_shift.h) is the channeliser's: every stage behind it sees the shifted bins.
int tetra_wbrx_set_shift(tetra_wbrx_t* h, uint32_t inc) {
    if (!h) return TETRA_ERR_ARG;
    return tetra_chan_set_shift(h->chan, inc);
}

int tetra_wbrx_get_shift(tetra_wbrx_t* h, uint32_t* inc) {
    if (!h) return TETRA_ERR_ARG;
    return tetra_chan_get_shift(h->chan, inc);
}

// So is the input map (include/ext/tetra_iqcond.h): it acts on the capture's samples, in the channeliser's loads.
int tetra_wbrx_set_input_map(tetra_wbrx_t* h, const tetra_iq_map_t* map) {
    if (!h) return TETRA_ERR_ARG;
    return tetra_chan_set_input_map(h->chan, map);
}

int tetra_wbrx_get_input_map(tetra_wbrx_t* h, tetra_iq_map_t* map, int* is_set) {
    if (!h) return TETRA_ERR_ARG;
    return tetra_chan_get_input_map(h->chan, map, is_set);
}

// The carriers' own offsets (include/ext/tetra_carrier_offset.h) are the selecting resampler's.  Like a retune, the setter works on the
// caller's stream between two process calls: behind the last call (ev_done), and the next call behind it (ev_done again).
int tetra_wbrx_set_carrier_offsets(tetra_wbrx_t* h, const uint32_t* inc, void* hip_stream) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h || !inc) return TETRA_ERR_ARG;
    tetra_resamp* rs = h->rs;
    bool same = true, any = false;
    for (int j = 0; j < h->n_bins; j++) {
        same = same && inc[j] == (rs->inc.empty() ? 0u : rs->inc[(size_t)j]);
        any = any || inc[j] != 0;
    }
    if (same) return TETRA_OK;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (!any) return resamp_impl::set_mix(rs, inc, nullptr, s);      // the un-mixed kernels again: nothing to upload
    DeviceGuard g(h->device);
    if (!g.ok) return TETRA_ERR_NO_DEVICE;
    std::vector<int32_t> words(resamp_impl::mix_words(rs));
    resamp_impl::mix_fill(rs, inc, words.data());
    // the tables in force are read by the last call's resampler: the new ones go in behind that call
    if (h->done_recorded) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_done, 0));
    int32_t* d_words = nullptr;
    hipError_t e = hipSuccess;
    const int k = h->mix_to_device.push(words.data(), (int)words.size(), (int)words.size(), s, &d_words, &e);
    if (k < 0) HIP_TRY(h, e);
    if (h->all) {      // from now on the selecting resampler, as after a first retune: the delay line already holds every bin in order
        (void)retune_impl::resamp_narrow_units(rs);
        h->all = false;
    }
    const int rc = resamp_impl::set_mix(rs, inc, d_words, s);
    if (rc == TETRA_ERR_HIP) h->last_hip = rs->last_hip;
    hipError_t late = h->mix_to_device.done(k, 0, s);
    if (late == hipSuccess) late = hipEventRecord(h->ev_done, s);
    if (late == hipSuccess) h->done_recorded = true;
    if (rc != TETRA_OK) return rc;
    HIP_TRY(h, late);
    return TETRA_OK;
}

int tetra_wbrx_get_carrier_offsets(tetra_wbrx_t* h, uint32_t* inc) {
    if (no_device()) return TETRA_ERR_NO_DEVICE;
    if (!h || !inc) return TETRA_ERR_ARG;
    const tetra_resamp* rs = h->rs;
    for (int j = 0; j < h->n_bins; j++) inc[j] = rs->inc.empty() ? 0u : rs->inc[(size_t)j];
    return TETRA_OK;
}

// round(offset_hz . decimation / sample_rate_hz . 2^32) mod 2^32, by tetra_chan_shift_from_hz's rules
uint32_t tetra_wbrx_carrier_offset_from_hz(double offset_hz, double sample_rate_hz, int decimation) {
    if (decimation < 1) return 0;
    return tetra_chan_shift_from_hz(offset_hz * (double)decimation, sample_rate_hz);
}

int tetra_wbrx_stage_ms(tetra_wbrx_t* h, float ms[2]) {
    if (!h || !ms || h->calls == 0) return TETRA_ERR_ARG;
    TETRA_TRY(tetra_chan_last_kernel_ms(h->chan, &ms[0]));
    return tetra_resamp_last_kernel_ms(h->rs, &ms[1]);
}

}  // extern "C"
