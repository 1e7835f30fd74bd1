"""ctypes binding of the wideband receiver (include/tetra_wbrx.h): one SDR capture in, the receive chain's blocks per carrier out."""
import ctypes as C
import functools

import numpy as np

from . import binding as B
from ._ffi import P, call, declare, f64, i32, i64, ptr, stream_ptr, u32, vp
from .binding import load_library
from .chan_binding import ChanConfig, IqMap, _get_input_map, _set_input_map, input_map_from_stats, iq_stats
from .rx_binding import HandoverParams, RxChain, RxConfig, gap_params_arg, handover_params_arg
from .rx_binding import _lib as _rx_lib


class WbrxConfig(C.Structure):
    _fields_ = [("chan", ChanConfig), ("interp", C.c_int32), ("decim", C.c_int32), ("taps_per_phase", C.c_int32), ("n_bins", C.c_int32),
                ("resamp_cutoff_rel", C.c_double), ("resamp_kaiser_beta", C.c_double), ("bins", C.c_void_p), ("rx", RxConfig)]


# include/tetra_wbrx.h
SIGNATURES = {
    "tetra_wbrx_default_config": (i32, [P(WbrxConfig)]),
    "tetra_wbrx_create": (i32, [P(WbrxConfig), P(vp)]),
    "tetra_wbrx_destroy": (i32, [vp]),
    "tetra_wbrx_reset": (i32, [vp]),
    "tetra_wbrx_process_device": (i32, [vp, vp, i32, vp]),
    "tetra_wbrx_process_device_cs16": (i32, [vp, vp, i32, vp]),
    "tetra_wbrx_process_device_cs8": (i32, [vp, vp, i32, vp]),
    "tetra_wbrx_process": (i32, [vp, vp, i32]),
    "tetra_wbrx_process_cs16": (i32, [vp, vp, i32]),
    "tetra_wbrx_rx": (vp, [vp]),
    "tetra_wbrx_bins": (i32, [vp, vp]),
    "tetra_wbrx_frames_device": (i32, [vp, i32, P(vp), P(i32), vp]),
    "tetra_wbrx_bin_power": (i32, [vp, vp]),
    "tetra_wbrx_stage_ms": (i32, [vp, P(C.c_float * 2)]),
}
# include/tetra_shift.h (the frequency-shifted bank): the wideband receiver's share
SHIFT_SIGNATURES = {
    "tetra_wbrx_set_shift": (i32, [vp, u32]),
    "tetra_wbrx_get_shift": (i32, [vp, P(u32)]),
}
# include/tetra_retune.h (carrier slots that move while the stream runs): the wideband receiver's share
RETUNE_SIGNATURES = {
    "tetra_wbrx_retune": (i32, [vp, vp, vp]),
    "tetra_wbrx_retune_count": (i32, [vp, P(i64), P(i64)]),
}
# include/ext/tetra_iqcond.h (conditioning of the capture): the wideband receiver's share
IQCOND_ABI = {
    "tetra_wbrx_set_input_map": (i32, [vp, P(IqMap)]),
    "tetra_wbrx_get_input_map": (i32, [vp, P(IqMap), P(i32)]),
}
# include/ext/tetra_handover.h (a moved slot inherits frame timing, cell and clock from a donor slot): the wideband receiver's share
HANDOVER_ABI = {"tetra_wbrx_retune_from": (i32, [vp, vp, vp, P(HandoverParams), vp])}
# include/ext/tetra_carrier_offset.h (an offset per carrier slot, mixed out in the selecting resampler)
CARRIER_OFFSET_ABI = {
    "tetra_wbrx_set_carrier_offsets": (i32, [vp, vp, vp]),
    "tetra_wbrx_get_carrier_offsets": (i32, [vp, vp]),
    "tetra_wbrx_carrier_offset_from_hz": (u32, [f64, f64, i32]),
}
WBRX_EXPORTS, WBRX_SHIFT_EXPORTS, WBRX_RETUNE_EXPORTS = list(SIGNATURES), list(SHIFT_SIGNATURES), list(RETUNE_SIGNATURES)
WBRX_HANDOVER_EXPORTS = list(HANDOVER_ABI)
# include/ext/tetra_gap.h (missing capture samples: the slots keep frame timing, cell and clock): the wideband receiver's share
GAP_ABI = {
    "tetra_wbrx_gap": (i32, [vp, i64, P(HandoverParams), P(i64), vp]),
    "tetra_wbrx_process_device_at": (i32, [vp, vp, i32, i32, i64, P(HandoverParams), vp]),
}
WBRX_GAP_EXPORTS = list(GAP_ABI)
IQ_FMT_C64, IQ_FMT_CS16, IQ_FMT_CS8 = range(3)          # TETRA_IQ_FMT_* (include/ext/tetra_iqcond.h)


@functools.lru_cache(None)
def _lib():
    # (a TETRA_DEMOD_LIB override may be an older build without the shift, the retune and the input map)
    return declare(load_library(), {**SIGNATURES, **SHIFT_SIGNATURES, **RETUNE_SIGNATURES, **IQCOND_ABI, **HANDOVER_ABI, **CARRIER_OFFSET_ABI, **GAP_ABI},
                   optional=WBRX_SHIFT_EXPORTS + WBRX_RETUNE_EXPORTS + list(IQCOND_ABI) + WBRX_HANDOVER_EXPORTS + list(CARRIER_OFFSET_ABI) + WBRX_GAP_EXPORTS)


def carrier_offset_from_hz(offset_hz, sample_rate_hz, decimation):
    """tetra_wbrx_carrier_offset_from_hz: the increment (2^-32 cycles per channeliser frame) of a carrier `offset_hz` above its bin's
    centre; negative offsets wrap."""
    return int(_lib().tetra_wbrx_carrier_offset_from_hz(float(offset_hz), float(sample_rate_hz), int(decimation)))


def default_config():
    cfg = WbrxConfig()
    call(_lib().tetra_wbrx_default_config, C.byref(cfg))
    return cfg


class _ChainView(RxChain):
    """The chain inside a WidebandRx (tetra_wbrx_rx): every RxChain reader (fetch, cells, sync_states, stage_ms, rows_device,
    bits_device, deliver ...) as it is.  It does not own the handle: close() only detaches it, and process / reset are refused --
    the wideband handle feeds and resets its chain."""

    def __init__(self, handle, n_channels, max_samples):          # (RxChain's owning constructor is not run)
        self._lib = _rx_lib()
        self._h = C.c_void_p(handle)
        self.n_channels, self.max_samples = n_channels, max_samples
        self.max_rows = int(self._lib.tetra_rx_max_rows(self._h))

    def close(self):
        self._h = None
        self._close_pool()

    def reset(self):
        raise TypeError("the wideband receiver's chain is reset through WidebandRx.reset()")

    def reset_channels(self, channels, stream=None):
        raise TypeError("the wideband receiver's slots are restarted through WidebandRx.retune()")

    def handover_channels(self, channels, donors, window=None, max_slots=None, stream=None):
        raise TypeError("the wideband receiver's slots are handed over through WidebandRx.retune(bins, donors=...)")

    def resume(self, elapsed_bits, channels=None, window=None, max_slots=None, stream=None):
        raise TypeError("the wideband receiver's slots resume through WidebandRx.gap() or process_device_at()")

    def process(self, iq):
        raise TypeError("the wideband receiver's chain is fed through WidebandRx.process*()")

    process_device = process


class _DeviceArray:
    """A device buffer as __cuda_array_interface__, for torch.as_tensor (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


class WidebandRx:
    """An SDR capture in, the decoded blocks of the carriers on `bins` out: channeliser (M bins) -> selecting 18 / 25 resampler ->
    receive chain on one GPU.  `.rx` is the chain (an RxChain view); a block's channel is the carrier's index into `bins`.  shift:
    the channeliser's frequency shift (include/tetra_shift.h, 2^-32 cycles per input sample) for carriers that share one offset from
    the bins' centres, e.g. chan_binding.shift_from_hz(12500, 20e6) for half a bin.  Extended deliveries (ext/tetra_rx_out_ext.h) need
    nothing here: `.rx.set_snapshot(mask)` and `.rx.deliver(..., extras=mask)` work on the chain tetra_wbrx_rx hands out.
    offsets_hz: per slot the carrier's own offset from its (shifted) bin centre in hertz at the capture rate n_channels x 25 kHz
    (include/ext/tetra_carrier_offset.h); set_offsets takes increments or hertz later."""

    def __init__(self, bins, n_channels=800, taps_per_channel=8, decimation=None, max_in=1 << 20, device=-1, chan_cutoff_rel=1.2,
                 chan_flags=0, interp=18, decim=25, taps_per_phase=16, resamp_cutoff_rel=1.0, resamp_kaiser_beta=6.0, kinds=0, flags=0,
                 demod_flags=0, shift=0, offsets_hz=None, **params):
        self._lib = _lib()
        cfg = default_config()
        cfg.chan.n_channels, cfg.chan.taps_per_channel = n_channels, taps_per_channel
        cfg.chan.decimation = decimation if decimation is not None else n_channels // 2
        cfg.chan.max_in, cfg.chan.device, cfg.chan.cutoff_rel, cfg.chan.reserved = max_in, device, chan_cutoff_rel, chan_flags
        cfg.interp, cfg.decim, cfg.taps_per_phase = interp, decim, taps_per_phase
        cfg.resamp_cutoff_rel, cfg.resamp_kaiser_beta = resamp_cutoff_rel, resamp_kaiser_beta
        keep = np.ascontiguousarray(np.asarray(bins, np.int64).astype(np.int32).reshape(-1))
        cfg.n_bins = keep.size
        cfg.bins = keep.ctypes.data if keep.size else None
        cfg.rx.kinds, cfg.rx.flags, cfg.rx.demod.flags = kinds, flags, demod_flags
        for k, v in params.items():
            if k not in B.PARAMS:
                raise TypeError("unknown parameter %r" % k)
            setattr(cfg.rx.demod, k, v)
        self.M, self.D, self.max_in, self.n_bins = n_channels, cfg.chan.decimation, max_in, int(keep.size)
        h = C.c_void_p()
        call(self._lib.tetra_wbrx_create, C.byref(cfg), C.byref(h))
        self._h = h
        max_samples = int(((self.D - 1 + max_in) // self.D) * interp // decim + 1)
        self.rx = _ChainView(self._lib.tetra_wbrx_rx(h), self.n_bins, max_samples)
        if shift:
            self.set_shift(shift)
        if offsets_hz is not None:
            self.set_offsets(hz=offsets_hz)

    def set_offsets(self, inc=None, hz=None, stream=None):
        """tetra_wbrx_set_carrier_offsets: per slot an offset `inc` (2^-32 cycles per channeliser frame) or `hz` (hertz, at the capture rate
        n_channels x 25 kHz); between process calls, enqueued on `stream`, from the next call on.  Neither: all zero (the default)."""
        if inc is not None and hz is not None:
            raise ValueError("offsets are given as increments or in hertz, not both")
        if hz is not None:
            hz = np.asarray(hz, np.float64).reshape(-1)
            inc = [carrier_offset_from_hz(f, self.M * 25000.0, self.D) for f in hz]
        new = np.zeros(self.n_bins, np.uint32) if inc is None else np.ascontiguousarray(np.asarray(inc, np.int64).reshape(-1) & 0xffffffff).astype(np.uint32)
        if new.size != self.n_bins:
            raise ValueError("set_offsets takes exactly %d offsets" % self.n_bins)
        call(self._lib.tetra_wbrx_set_carrier_offsets, self._h, ptr(new), stream_ptr(stream))

    def offsets(self):
        """The offsets in force (tetra_wbrx_get_carrier_offsets), uint32 [n_bins]."""
        out = np.zeros(max(self.n_bins, 1), np.uint32)
        call(self._lib.tetra_wbrx_get_carrier_offsets, self._h, ptr(out))
        return out[:self.n_bins]

    def set_shift(self, inc):
        """tetra_wbrx_set_shift: forwards to the channeliser; between process calls, from the next call's first frame."""
        call(self._lib.tetra_wbrx_set_shift, self._h, int(inc) & 0xffffffff)

    def get_shift(self):
        v = C.c_uint32(0)
        call(self._lib.tetra_wbrx_get_shift, self._h, C.byref(v))
        return int(v.value)

    def set_input_map(self, m):
        """tetra_wbrx_set_input_map (include/ext/tetra_iqcond.h): forwards to the channeliser -- six coefficients (m00, m01, m10, m11, c0, c1)
        or None for the un-conditioned kernels; between process calls, from the next call's first new sample."""
        _set_input_map(self._lib.tetra_wbrx_set_input_map, self._h, m)

    def get_input_map(self):
        """The six coefficients in force, or None if no map is set."""
        return _get_input_map(self._lib.tetra_wbrx_get_input_map, self._h)

    def estimate_input_map(self, x, n=None, stream=None):
        """The blind estimate from a stretch of the capture on the device (iq_stats -> input_map_from_stats), set on this handle and
        returned.  x: as process_device takes it; n: samples (default: all of the tensor).  The handle's map stays as it was if the
        solver refuses the statistics."""
        m = input_map_from_stats(iq_stats(x, n, stream))
        self.set_input_map(m)
        return m

    def retune(self, bins, stream=None, donors=None, window=None, max_slots=None, offsets=None):
        """tetra_wbrx_retune: slot j receives bins[j] from the next process call on.  Slots whose bin stays are untouched; every other
        slot starts afresh on its new bin.  Enqueued on `stream` (the one the process calls use), not waited for.
        donors (tetra_wbrx_retune_from, include/ext/tetra_handover.h): per slot a donor slot whose bin stays, or -1 -- a moving slot with
        a donor inherits its frame timing, cell and TDMA clock (window / max_slots: None = the header's defaults).
        offsets: the slots' new offsets (set_offsets' increments), set on the same stream ahead of the retune; None keeps every slot's."""
        new = np.ascontiguousarray(np.asarray(bins, np.int64).astype(np.int32).reshape(-1))
        if new.size != self.n_bins:
            raise ValueError("retune takes exactly %d bins" % self.n_bins)
        if offsets is not None:
            self.set_offsets(offsets, stream=stream)
        if donors is None:
            call(self._lib.tetra_wbrx_retune, self._h, ptr(new), stream_ptr(stream))
            return
        dn = np.ascontiguousarray(np.asarray(donors, np.int64).astype(np.int32).reshape(-1))
        if dn.size != self.n_bins:
            raise ValueError("retune takes a donor (or -1) per slot")
        call(self._lib.tetra_wbrx_retune_from, self._h, ptr(new), ptr(dn), handover_params_arg(window, max_slots), stream_ptr(stream))

    def handover_status(self, first=0, count=None):
        """The carrier slots' hand-over status (RxChain.handover_status of the chain)."""
        return self.rx.handover_status(first, count)

    def retune_count(self):
        """-> (accepted retunes, slots they moved) since create."""
        a, b = C.c_int64(0), C.c_int64(0)
        call(self._lib.tetra_wbrx_retune_count, self._h, C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def close(self):
        if getattr(self, "rx", None) is not None:
            self.rx.close()
        if getattr(self, "_h", None):
            self._lib.tetra_wbrx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        call(self._lib.tetra_wbrx_reset, self._h)

    def process(self, x):
        """Host capture: complex64 [n], or int16 interleaved I / Q ([n][2] or [2 n]) -> tetra_wbrx_process / _process_cs16."""
        x = np.asarray(x)
        if x.dtype == np.int16:
            x = np.ascontiguousarray(x).reshape(-1)
            call(self._lib.tetra_wbrx_process_cs16, self._h, ptr(x), x.size // 2)
        else:
            x = np.ascontiguousarray(x, np.complex64).reshape(-1)
            call(self._lib.tetra_wbrx_process, self._h, ptr(x), x.size)

    def process_device(self, d_x, n_in=None, stream=None):
        """Device capture: the entry point follows the tensor's dtype (complex64, or interleaved I / Q pairs int16 / int8, as
        Channeliser.process_device).  n_in: samples (default: all of the tensor)."""
        dt = str(getattr(d_x, "dtype", ""))
        name = {"torch.int16": "tetra_wbrx_process_device_cs16", "torch.int8": "tetra_wbrx_process_device_cs8"}.get(dt, "tetra_wbrx_process_device")
        if n_in is None:
            n_in = d_x.numel() // 2 if name != "tetra_wbrx_process_device" else d_x.numel()
        call(getattr(self._lib, name), self._h, ptr(d_x), int(n_in), stream_ptr(stream))

    def gap(self, n_lost, window=None, max_slots=None, stream=None):
        """tetra_wbrx_gap (include/ext/tetra_gap.h): `n_lost` capture samples are missing between the last process call and the next.  The
        front end restarts as after reset() -- with no host synchronisation, and keeping bins, shift, offsets and input map -- and every
        slot that was locked keeps its scrambling code and its TDMA clock, advanced by the slots that passed.  Enqueued on `stream` (the
        one the process calls use).  -> the elapsed bits the lost samples stand for; handover_status() says what became of each slot."""
        g = C.c_int64(0)
        call(self._lib.tetra_wbrx_gap, self._h, int(n_lost), gap_params_arg(window, max_slots), C.byref(g), stream_ptr(stream))
        return int(g.value)

    def process_device_at(self, d_x, first_index, n_in=None, window=None, max_slots=None, stream=None):
        """tetra_wbrx_process_device_at: process_device for a buffer whose first sample has the driver's sample index `first_index`.  The
        first call sets the origin; an index ahead of the expected one is a gap() of the difference, one behind it is refused."""
        dt = str(getattr(d_x, "dtype", ""))
        fmt = {"torch.int16": IQ_FMT_CS16, "torch.int8": IQ_FMT_CS8}.get(dt, IQ_FMT_C64)
        if n_in is None:
            n_in = d_x.numel() // 2 if fmt != IQ_FMT_C64 else d_x.numel()
        call(self._lib.tetra_wbrx_process_device_at, self._h, ptr(d_x), fmt, int(n_in), int(first_index), gap_params_arg(window, max_slots), stream_ptr(stream))

    def bins(self):
        out = np.zeros(max(self.n_bins, 1), np.int32)
        call(self._lib.tetra_wbrx_bins, self._h, ptr(out))
        return out[:self.n_bins]

    def frames_device(self, which=0, stream=None):
        """-> (device pointer, n_frames) of the resampled carrier IQ [n_frames][n_bins] complex64 of the latest (0) / previous (1) call."""
        p, n = C.c_void_p(), C.c_int(0)
        call(self._lib.tetra_wbrx_frames_device, self._h, int(which), C.byref(p), C.byref(n), stream_ptr(stream))
        return p.value, n.value

    def frames(self, which=0, stream=None):
        """The same as a torch tensor [n_frames][n_bins] complex64 on the handle's GPU: a view, valid until the next-but-one call."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream()
        p, n = self.frames_device(which, stream)
        if n == 0:
            return torch.zeros((0, self.n_bins), dtype=torch.complex64, device=stream.device)
        return torch.as_tensor(_DeviceArray(p, (n, self.n_bins), "<c8"), device=stream.device)

    def links(self, first=0, count=None):
        """The carrier slots' link figures (RxChain.links of the chain; needs FLAG_BITERR in `flags`).  A retune zeroes a moved slot's."""
        return self.rx.links(first, count)

    def set_sync_tolerance(self, tol):
        """The tolerant lock of the carrier slots' synchroniser (RxChain.set_sync_tolerance of the chain); between process calls."""
        self.rx.set_sync_tolerance(tol)

    def sync_misses(self, first=0, count=None):
        """The carrier slots' miss counters (RxChain.sync_misses of the chain).  A retune zeroes a moved slot's."""
        return self.rx.sync_misses(first, count)

    def set_aach_min_margin(self, min_margin):
        """The margin from which the carrier slots' maximum-likelihood AACH rows are accepted (RxChain.set_aach_min_margin of the chain;
        needs FLAG_SOFT | FLAG_AACH_SOFT in `flags`)."""
        self.rx.set_aach_min_margin(min_margin)

    def fetch_aach_margin(self, which=0):
        """The AACH rows' margins (RxChain.fetch_aach_margin of the chain)."""
        return self.rx.fetch_aach_margin(which)

    # include/ext/tetra_traffic.h by carrier slot: RxChain's methods of the chain (a retune leaves a slot's table entries as they are)
    def enable_traffic(self, max_rows=None):
        self.rx.enable_traffic(max_rows)

    def set_traffic(self, table, first=0, stream=None):
        self.rx.set_traffic(table, first, stream)

    def traffic(self, first=0, count=None):
        return self.rx.traffic(first, count)

    def fetch_traffic(self, tch_kind, which=0, biterr=False):
        return self.rx.fetch_traffic(tch_kind, which, biterr)

    def traffic_rows_device(self, tch_kind, which=0, stream=None):
        return self.rx.traffic_rows_device(tch_kind, which, stream)

    def bin_power(self):
        out = np.zeros(self.M, np.float32)
        call(self._lib.tetra_wbrx_bin_power, self._h, ptr(out))
        return out

    def stage_ms(self):
        ms = (C.c_float * 2)()
        call(self._lib.tetra_wbrx_stage_ms, self._h, C.byref(ms))
        return [float(v) for v in ms]
