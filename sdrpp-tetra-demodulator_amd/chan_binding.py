"""ctypes binding of the channeliser front-end C ABI (include/tetra_chan.h)."""
import ctypes as C
import functools

import numpy as np

from ._ffi import P, call, declare, f64, i32, ptr, stream_ptr, u32, vp
from .binding import load_library


class ChanConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int32), ("taps_per_channel", C.c_int32), ("decimation", C.c_int32),
                ("max_in", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32),
                ("cutoff_rel", C.c_double), ("prototype", C.c_void_p)]


class ResampConfig(C.Structure):
    _fields_ = [("n_channels", C.c_int32), ("interp", C.c_int32), ("decim", C.c_int32), ("taps_per_phase", C.c_int32),
                ("max_in", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("cutoff_rel", C.c_double), ("kaiser_beta", C.c_double), ("prototype", C.c_void_p)]


# include/tetra_chan.h
SIGNATURES = {
    "tetra_chan_default_config": (i32, [P(ChanConfig)]),
    "tetra_chan_create": (i32, [P(ChanConfig), P(vp)]),
    "tetra_chan_destroy": (i32, [vp]),
    "tetra_chan_frames_for": (i32, [vp, i32]),
    "tetra_chan_process_device": (i32, [vp, vp, i32, vp, P(i32), vp]),
    "tetra_chan_process_device_cs16": (i32, [vp, vp, i32, vp, P(i32), vp]),
    "tetra_chan_process_device_cs8": (i32, [vp, vp, i32, vp, P(i32), vp]),
    "tetra_chan_process": (i32, [vp, vp, i32, vp, P(i32)]),
    "tetra_chan_reset": (i32, [vp]),
    "tetra_chan_get_prototype": (i32, [vp, vp]),
    "tetra_chan_last_kernel_ms": (i32, [vp, P(C.c_float)]),
    "tetra_resamp_default_config": (i32, [P(ResampConfig)]),
    "tetra_resamp_create": (i32, [P(ResampConfig), P(vp)]),
    "tetra_resamp_destroy": (i32, [vp]),
    "tetra_resamp_frames_for": (i32, [vp, i32]),
    "tetra_resamp_process_device": (i32, [vp, vp, i32, vp, P(i32), vp]),
    "tetra_resamp_process": (i32, [vp, vp, i32, vp, P(i32)]),
    "tetra_resamp_reset": (i32, [vp]),
    "tetra_resamp_get_prototype": (i32, [vp, vp]),
    "tetra_resamp_last_kernel_ms": (i32, [vp, P(C.c_float)]),
}
# include/tetra_shift.h (the frequency-shifted bank): the channeliser's share
SHIFT_SIGNATURES = {
    "tetra_chan_set_shift": (i32, [vp, u32]),
    "tetra_chan_get_shift": (i32, [vp, P(u32)]),
    "tetra_chan_shift_from_hz": (u32, [f64, f64]),
}
CHAN_EXPORTS = [n for n in SIGNATURES if n.startswith("tetra_chan_")]
RESAMP_EXPORTS = [n for n in SIGNATURES if n.startswith("tetra_resamp_")]
CHAN_SHIFT_EXPORTS = list(SHIFT_SIGNATURES)


class IqMap(C.Structure):
    """tetra_iq_map_t (include/ext/tetra_iqcond.h): (yr, yi) = (m00 xr + m01 xi + c0, m10 xr + m11 xi + c1)."""
    _fields_ = [(n, C.c_float) for n in ("m00", "m01", "m10", "m11", "c0", "c1")]

    def astuple(self):
        return tuple(float(getattr(self, n)) for n, _ in self._fields_)


class IqStats(C.Structure):
    """tetra_iq_stats_t: the sums of n samples in the converted samples' unit."""
    _fields_ = [("n", C.c_int64)] + [(n, C.c_double) for n in ("s_i", "s_q", "s_ii", "s_qq", "s_iq")]

    def astuple(self):
        return (int(self.n),) + tuple(float(getattr(self, n)) for n, _ in self._fields_[1:])


# include/ext/tetra_iqcond.h (conditioning of the capture): the channeliser's share and the two handle-free entry points
IQCOND_ABI = {
    "tetra_chan_set_input_map": (i32, [vp, P(IqMap)]),
    "tetra_chan_get_input_map": (i32, [vp, P(IqMap), P(i32)]),
    "tetra_iq_stats_device": (i32, [vp, i32, C.c_longlong, P(IqStats), vp]),
    "tetra_iq_map_from_stats": (i32, [P(IqStats), P(IqMap)]),
}
IQ_FMT_C64, IQ_FMT_CS16, IQ_FMT_CS8 = 0, 1, 2


@functools.lru_cache(None)
def _lib():
    # (a TETRA_DEMOD_LIB override may be an older build without the shift or the input map)
    return declare(load_library(), {**SIGNATURES, **SHIFT_SIGNATURES, **IQCOND_ABI}, optional=CHAN_SHIFT_EXPORTS + list(IQCOND_ABI))


def shift_from_hz(shift_hz, sample_rate_hz):
    """tetra_chan_shift_from_hz: the increment (2^-32 cycles per input sample) of a shift in hertz; negative shifts wrap."""
    return int(_lib().tetra_chan_shift_from_hz(float(shift_hz), float(sample_rate_hz)))


def as_iq_map(m):
    """None stays None; an IqMap is passed through; six numbers (m00, m01, m10, m11, c0, c1) become one."""
    if m is None or isinstance(m, IqMap):
        return m
    vals = [float(v) for v in m]
    if len(vals) != 6:
        raise ValueError("an input map has six coefficients: m00, m01, m10, m11, c0, c1")
    return IqMap(*vals)


def _set_input_map(fn, handle, m):
    m = as_iq_map(m)
    call(fn, handle, None if m is None else C.byref(m))


def _get_input_map(fn, handle):
    m, on = IqMap(), C.c_int(0)
    call(fn, handle, C.byref(m), C.byref(on))
    return m.astuple() if on.value else None


def iq_stats(x, n=None, stream=None):
    """tetra_iq_stats_device: the sums (IqStats) of a capture on the device -- a torch tensor, complex64 [n] or interleaved I / Q pairs
    int16 / int8 [n][2] (as Channeliser.process_device); n: samples (default: all of the tensor)."""
    dt = str(getattr(x, "dtype", ""))
    fmt = {"torch.int16": IQ_FMT_CS16, "torch.int8": IQ_FMT_CS8}.get(dt, IQ_FMT_C64)
    if n is None:
        n = x.numel() // 2 if fmt != IQ_FMT_C64 else x.numel()
    out = IqStats()
    call(_lib().tetra_iq_stats_device, ptr(x) if n else None, fmt, int(n), C.byref(out), stream_ptr(stream))
    return out


def input_map_from_stats(stats):
    """tetra_iq_map_from_stats (host only): the six coefficients that remove the DC offset and decorrelate and equalise I and Q."""
    if not isinstance(stats, IqStats):
        stats = IqStats(*stats)
    m = IqMap()
    call(_lib().tetra_iq_map_from_stats, C.byref(stats), C.byref(m))
    return m.astuple()


class Channeliser:
    """M-channel analysis filter bank on one GPU; emits time-major frames [frames][M] complex64.  shift: the frequency shift of
    include/tetra_shift.h in 2^-32 cycles per input sample (0 = off), for carriers off the bins' centres by one common offset."""

    FLAG_VALU_DFT = 1      # TETRA_CHAN_FLAG_VALU_DFT: keep the direct-sum DFT kernel where a faster form exists (M = 800)
    FLAG_MATRIX_DFT = 2    # TETRA_CHAN_FLAG_MATRIX_DFT: M = 800 at D = M / 2 as 25 x 32 matrix products (round 4's kernel) instead of the mixed-radix FFT

    def __init__(self, n_channels=800, taps_per_channel=8, decimation=None, max_in=1 << 20, device=-1, cutoff_rel=1.2,
                 prototype=None, flags=0, shift=0):
        self._lib = _lib()
        cfg = ChanConfig()
        self._lib.tetra_chan_default_config(C.byref(cfg))
        cfg.n_channels = n_channels
        cfg.taps_per_channel = taps_per_channel
        cfg.decimation = decimation if decimation is not None else n_channels // 2
        cfg.max_in = max_in
        cfg.device = device
        cfg.cutoff_rel = cutoff_rel
        cfg.reserved = flags
        keep = None
        if prototype is not None:
            keep = np.ascontiguousarray(prototype, np.float32)
            cfg.prototype = keep.ctypes.data
        self.M, self.P, self.D = n_channels, taps_per_channel, cfg.decimation
        h = C.c_void_p()
        call(self._lib.tetra_chan_create, C.byref(cfg), C.byref(h))
        self._h = h
        if shift:
            self.set_shift(shift)

    def set_shift(self, inc):
        """tetra_chan_set_shift: between process calls; takes effect from the next call's first frame, keeps the phase reference."""
        call(self._lib.tetra_chan_set_shift, self._h, int(inc) & 0xffffffff)

    def get_shift(self):
        v = C.c_uint32(0)
        call(self._lib.tetra_chan_get_shift, self._h, C.byref(v))
        return int(v.value)

    def set_input_map(self, m):
        """tetra_chan_set_input_map (include/ext/tetra_iqcond.h): six coefficients (m00, m01, m10, m11, c0, c1) or an IqMap; None returns
        the handle to the un-conditioned kernels.  Between process calls; from the next call's first new sample."""
        _set_input_map(self._lib.tetra_chan_set_input_map, self._h, m)

    def get_input_map(self):
        """The six coefficients in force, or None if no map is set."""
        return _get_input_map(self._lib.tetra_chan_get_input_map, self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tetra_chan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frames_for(self, n_in):
        return int(self._lib.tetra_chan_frames_for(self._h, int(n_in)))

    def process(self, x):
        x = np.ascontiguousarray(x, np.complex64)
        nf = self.frames_for(x.shape[0])
        out = np.zeros((max(nf, 1), self.M), np.complex64)
        got = C.c_int(0)
        call(self._lib.tetra_chan_process, self._h, ptr(x), x.shape[0], ptr(out), C.byref(got))
        return out[: got.value]

    def process_device(self, d_x, n_in, d_out, stream=None):
        got = C.c_int(0)
        # the input format follows the tensor: complex64, or interleaved I / Q pairs [n][2] int16 / int8 (tetra_chan_process_device_cs16 / _cs8)
        name = {"torch.int16": "tetra_chan_process_device_cs16", "torch.int8": "tetra_chan_process_device_cs8"}.get(str(getattr(d_x, "dtype", "")),
                                                                                                                  "tetra_chan_process_device")
        call(getattr(self._lib, name), self._h, ptr(d_x), int(n_in), ptr(d_out), C.byref(got), stream_ptr(stream))
        return got.value

    def reset(self):
        call(self._lib.tetra_chan_reset, self._h)

    def prototype(self):
        h = np.zeros(self.M * self.P, np.float32)
        self._lib.tetra_chan_get_prototype(self._h, ptr(h))
        return h

    def last_kernel_ms(self):
        v = C.c_float(0)
        call(self._lib.tetra_chan_last_kernel_ms, self._h, C.byref(v))
        return v.value


class Resampler:
    """Rational resampler I / DN on time-major frames [n][C] complex64 on one GPU (include/tetra_chan.h, tetra_resamp_*): the
    18 / 25 stage between the 50 ksps channeliser and a demodulator at the plugin's 36 ksps."""

    FLAG_GENERIC = 1      # TETRA_RESAMP_FLAG_GENERIC: keep the run-time-ratio kernel where a specialised one exists
    FLAG_NARROW_UNITS = 2 # TETRA_RESAMP_FLAG_NARROW_UNITS: 8-byte lane units (one channel per lane) instead of 16-byte ones

    def __init__(self, n_channels=800, interp=18, decim=25, taps_per_phase=16, max_in=1 << 16, device=-1, cutoff_rel=1.0,
                 kaiser_beta=6.0, prototype=None, flags=0):
        self._lib = _lib()
        cfg = ResampConfig()
        self._lib.tetra_resamp_default_config(C.byref(cfg))
        cfg.n_channels, cfg.interp, cfg.decim, cfg.taps_per_phase = n_channels, interp, decim, taps_per_phase
        cfg.max_in, cfg.device, cfg.flags = max_in, device, flags
        cfg.cutoff_rel, cfg.kaiser_beta = cutoff_rel, kaiser_beta
        keep = None
        if prototype is not None:
            keep = np.ascontiguousarray(prototype, np.float32)
            assert keep.size == interp * taps_per_phase
            cfg.prototype = keep.ctypes.data
        self.C, self.I, self.DN, self.T = n_channels, interp, decim, taps_per_phase
        h = C.c_void_p()
        call(self._lib.tetra_resamp_create, C.byref(cfg), C.byref(h))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tetra_resamp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def frames_for(self, n_in):
        return int(self._lib.tetra_resamp_frames_for(self._h, int(n_in)))

    def process(self, x):
        x = np.ascontiguousarray(x, np.complex64).reshape(-1, self.C)
        nf = self.frames_for(x.shape[0])
        out = np.zeros((max(nf, 1), self.C), np.complex64)
        got = C.c_int(0)
        call(self._lib.tetra_resamp_process, self._h, ptr(x), x.shape[0], ptr(out), C.byref(got))
        return out[: got.value]

    def process_device(self, d_in, n_in, d_out, stream=None):
        got = C.c_int(0)
        call(self._lib.tetra_resamp_process_device, self._h, ptr(d_in), int(n_in), ptr(d_out), C.byref(got), stream_ptr(stream))
        return got.value

    def reset(self):
        call(self._lib.tetra_resamp_reset, self._h)

    def prototype(self):
        h = np.zeros(self.I * self.T, np.float32)
        self._lib.tetra_resamp_get_prototype(self._h, ptr(h))
        return h

    def last_kernel_ms(self):
        v = C.c_float(0)
        call(self._lib.tetra_resamp_last_kernel_ms, self._h, C.byref(v))
        return v.value
