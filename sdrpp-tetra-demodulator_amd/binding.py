"""ctypes binding of the C ABI (include/tetra_demod.h) -> libtetra_demod_hip.so.

Mirrors the reference's block interface for this path: one `Demodulator` = C copies of
PI4DQPSK -> DQPSKSymbolExtractor -> BitUnpacker (src/dsp/pi4dqpsk.h:27-81,
src/dsp/dqpsk_sym_extr.h:19-46, src/dsp/bit_unpacker.h:16-34) with init / process / reset /
setters.  There is no CPU fallback: if the HIP library is missing or no GPU is usable, every
call raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build
from ._ffi import P, TetraDemodError, call, check, declare, f64, i32, ptr, size_t, stream_ptr, vp  # noqa: F401

LAYOUT_CHANNEL_MAJOR = 0
LAYOUT_TIME_MAJOR = 1
FLAG_WIDE_WORKGROUPS, FLAG_NARROW_WORKGROUPS, FLAG_SMALL_WORKGROUPS = 16, 32, 64
FLAG_RETIRED_TWO_KERNEL = 1      # refused by tetra_demod_create since ABI 2
FLAG_KEEP_RRC_OUT = 2
FLAG_QUALITY = 4
FLAG_REFERENCE_QUIRKS = 8
FLAG_CONSTELLATION = 256         # keep the constellation diagram's 1024-symbol blocks per channel (Demod.constellation)
CONSTELLATION_SYMBOLS = 1024
FLAG_GENERIC_KERNEL = 128        # filters of 73 .. 129 taps / loops below 0.27 samples per symbol in the one-lane-per-channel kernel

PARAMS = dict(symbolrate=0, samplerate=1, rrc_tap_count=2, rrc_beta=3, agc_rate=4, costas_bandwidth=5,
              fll_bandwidth=6, omega_gain=7, mu_gain=8, omega_rel_limit=9)

ERR_OVERRUN = -8
IQ_CF32, IQ_CS16, IQ_CS8 = 0, 1, 2


class Config(C.Structure):
    _fields_ = [
        ("n_channels", C.c_int32), ("max_samples", C.c_int32), ("layout", C.c_int32), ("device", C.c_int32),
        ("symbolrate", C.c_double), ("samplerate", C.c_double),
        ("rrc_tap_count", C.c_int32), ("flags", C.c_int32),
        ("rrc_beta", C.c_double), ("agc_rate", C.c_double), ("costas_bandwidth", C.c_double),
        ("fll_bandwidth", C.c_double), ("omega_gain", C.c_double), ("mu_gain", C.c_double),
        ("omega_rel_limit", C.c_double),
        ("rrc_taps", C.c_void_p), ("bandedge_taps", C.c_void_p), ("interp_bank", C.c_void_p),
    ]


class ChannelState(C.Structure):
    _fields_ = [
        ("agc_gain", C.c_float), ("fll_phase", C.c_float), ("fll_freq", C.c_float),
        ("mu", C.c_float), ("omega", C.c_float), ("offset", C.c_int32),
        ("costas_phase", C.c_float), ("costas_freq", C.c_float), ("ph2", C.c_float), ("prev", C.c_int32),
        ("hist", C.c_float * 160), ("ybuf", C.c_float * 14), ("rrc_valid", C.c_int32),
        ("hist_far", C.c_float * 96),
    ]


# include/tetra_demod.h
SIGNATURES = {
    "tetra_demod_default_config": (i32, [P(Config)]),
    "tetra_demod_device_count": (i32, []),
    "tetra_demod_create": (i32, [P(Config), P(vp)]),
    "tetra_demod_destroy": (i32, [vp]),
    "tetra_demod_bits_stride_for": (i32, [vp, i32]),
    "tetra_demod_bits_stride": (i32, [i32]),
    "tetra_demod_process_device": (i32, [vp, vp, i32, vp, i32, vp, vp, vp]),
    "tetra_demod_process": (i32, [vp, vp, i32, vp, i32, vp, vp]),
    "tetra_demod_process_resident": (i32, [vp, vp, i32, vp, i32, vp, vp]),
    "tetra_demod_get_overruns": (i32, [vp, P(C.c_longlong)]),
    "tetra_demod_process_async": (i32, [vp, vp, i32, i32, vp, i32, vp]),
    "tetra_demod_wait": (i32, [vp]),
    "tetra_demod_host_alloc": (vp, [size_t]),
    "tetra_demod_host_free": (None, [vp]),
    "tetra_demod_reset": (i32, [vp, i32]),
    "tetra_demod_set_param": (i32, [vp, i32, f64]),
    "tetra_demod_set_rrc_params": (i32, [vp, i32, f64]),
    "tetra_demod_set_tables": (i32, [vp, vp, i32, vp, i32, vp]),
    "tetra_demod_get_state": (i32, [vp, i32, P(ChannelState)]),
    "tetra_demod_set_state": (i32, [vp, i32, P(ChannelState)]),
    "tetra_demod_get_tables": (i32, [vp, P(i32), vp, P(i32), vp, vp, vp]),
    "tetra_demod_bandedge_tap_count": (i32, [vp]),
    "tetra_demod_get_quality": (i32, [vp, vp, vp]),
    "tetra_demod_get_constellation": (i32, [vp, i32, i32, vp, vp]),
    "tetra_demod_debug_read_rrc_out": (i32, [vp, vp, i32]),
    "tetra_demod_last_kernel_ms": (i32, [vp, P(C.c_float)]),
    "tetra_demod_kernel_ms_history": (i32, [vp, i32, vp]),
    "tetra_demod_debug_selftest": (i32, [vp, vp, vp]),
    "tetra_demod_debug_mfma_selftest": (i32, [vp, i32, i32, vp, vp, vp]),
    "tetra_demod_strerror": (C.c_char_p, [i32]),
    "tetra_demod_last_hip_error": (i32, [vp]),
    "tetra_demod_abi_version": (i32, []),
    "tetra_demod_build_id": (C.c_char_p, []),
    "tetra_demod_device_info": (i32, [i32, P(i32), P(i32)]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def load_library(rebuild_if_stale=True):
    """Load libtetra_demod_hip.so (building it with hipcc when missing/stale).  Raises if impossible.
    When the process also uses torch on the GPU, `import torch` BEFORE calling this: torch bundles its own HIP runtime, this
    library links the system one, and the first one loaded serves both (a torch imported second finds no GPU)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    override = os.environ.get("TETRA_DEMOD_LIB")     # profiling scripts: an experimental build of the same ABI
    if override:
        path = os.path.abspath(override)
    elif rebuild_if_stale and _build.is_stale():
        path = _build.build()
    if not os.path.exists(path):
        raise RuntimeError("HIP library %s is missing; run __graft_entry__.build() (no CPU fallback exists)" % path)
    if not override and _build.lib_build_id(path) != _build.source_hash():
        # never run (or measure) a library built from other sources than the tree holds
        raise RuntimeError("HIP library %s was built from other sources than this tree holds (build id %s, sources %s); run "
                           "__graft_entry__.build()" % (path, _build.lib_build_id(path), _build.source_hash()))
    # (an override may be an older experimental build without the build id)
    _lib = declare(C.CDLL(path), SIGNATURES, optional=("tetra_demod_build_id",))
    return _lib


def device_info(device=0):
    """(shader clock in kHz, compute units) of a device."""
    clk, cus = C.c_int32(0), C.c_int32(0)
    call(load_library().tetra_demod_device_info, int(device), C.byref(clk), C.byref(cus))
    return int(clk.value), int(cus.value)


def default_config():
    cfg = Config()
    call(load_library().tetra_demod_default_config, C.byref(cfg))
    return cfg


def device_count():
    return int(load_library().tetra_demod_device_count())


def bits_stride(n_samples):
    """Handle-free row length: covers every handle at ~2 samples per symbol (tetra_demod_bits_stride); Demodulator.bits_stride
    is the one for a particular handle's rates."""
    return int(load_library().tetra_demod_bits_stride(int(n_samples)))


class Demodulator:
    """C batched reference chains on one GPU."""

    def __init__(self, n_channels=1, max_samples=65536, layout=LAYOUT_CHANNEL_MAJOR, device=-1,
                 rrc_taps=None, bandedge_taps=None, interp_bank=None, flags=0, **params):
        self._lib = load_library()
        cfg = default_config()
        cfg.n_channels = n_channels
        cfg.max_samples = max_samples
        cfg.layout = layout
        cfg.device = device
        cfg.flags = flags
        for k, v in params.items():
            if k not in PARAMS:
                raise TypeError("unknown parameter %r" % k)
            setattr(cfg, k, v)
        keep = []
        for name, arr in (("rrc_taps", rrc_taps), ("bandedge_taps", bandedge_taps), ("interp_bank", interp_bank)):
            if arr is not None:
                a = np.ascontiguousarray(arr, dtype=np.float32)
                keep.append(a)
                setattr(cfg, name, a.ctypes.data)
        self.cfg = cfg
        self.n_channels = n_channels
        self.max_samples = max_samples
        self.layout = layout
        h = C.c_void_p()
        call(self._lib.tetra_demod_create, C.byref(cfg), C.byref(h))
        self._h = h

    def _check(self, rc, fn):
        if rc:
            check(rc, fn, self._lib.tetra_demod_last_hip_error(self._h))

    def _call(self, fn, *args):
        """fn(handle, *args); a non-zero status raises with the handle's last HIP error."""
        rc = fn(self._h, *args)
        if rc:
            check(rc, fn, self._lib.tetra_demod_last_hip_error(self._h))

    def bits_stride(self, n_samples):
        """tetra_demod_bits_stride_for: the row length this handle's timing loop needs for calls of n_samples."""
        rc = int(self._lib.tetra_demod_bits_stride_for(self._h, int(n_samples)))
        if rc < 0:
            check(rc, self._lib.tetra_demod_bits_stride_for)
        return rc

    def overruns(self):
        """(channel, launch) events cut off at the row capacity since create (tetra_demod_get_overruns)."""
        v = C.c_longlong(0)
        self._call(self._lib.tetra_demod_get_overruns, C.byref(v))
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tetra_demod_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- PI4DQPSK::process + DQPSKSymbolExtractor::process + BitUnpacker::process --------------------
    def process(self, iq, want_sym=False, allow_overrun=False):
        """Host path.  iq complex64 [C][N] (channel-major) or [N][C] (time-major handle).
        Returns (bits u8 [C][stride], n_bits i32 [C], sym complex64 [C][stride/2] or None).  TETRA_ERR_OVERRUN (a poisoned
        channel filled its row; everything was delivered) raises unless allow_overrun; self.last_status keeps it."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        if iq.ndim == 1:
            iq = iq[None, :] if self.layout == LAYOUT_CHANNEL_MAJOR else iq[:, None]
        n = iq.shape[1] if self.layout == LAYOUT_CHANNEL_MAJOR else iq.shape[0]
        cdim = iq.shape[0] if self.layout == LAYOUT_CHANNEL_MAJOR else iq.shape[1]
        if cdim != self.n_channels:
            raise ValueError("expected %d channels, got %d" % (self.n_channels, cdim))
        stride = max(bits_stride(n), self.bits_stride(n))
        bits = np.zeros((self.n_channels, stride), np.uint8)
        nb = np.zeros(self.n_channels, np.int32)
        sym = np.zeros((self.n_channels, stride // 2), np.complex64) if want_sym else None
        rc = self._lib.tetra_demod_process(self._h, ptr(iq), n, ptr(bits), stride, ptr(nb), ptr(sym))
        self.last_status = rc
        if not (allow_overrun and rc == ERR_OVERRUN):
            self._check(rc, self._lib.tetra_demod_process)
        return bits, nb, sym

    def process_async(self, iq_ptr, iq_format, n_samples, bits_ptr, bits_stride_, n_bits_ptr):
        """tetra_demod_process_async on raw host addresses (page-locked buffers, e.g. torch pinned tensors' data_ptr() or
        host_alloc()); the buffers must stay alive and untouched until wait()."""
        self._call(self._lib.tetra_demod_process_async, int(iq_ptr), int(iq_format), int(n_samples), int(bits_ptr), int(bits_stride_),
                   int(n_bits_ptr))

    def wait(self):
        self._call(self._lib.tetra_demod_wait)

    def process_resident(self, d_iq, n_samples, d_bits, bits_stride_, d_n_bits, d_sym=None):
        """tetra_demod_process_resident: device buffers, the handle's own stream, returns when the launch is done."""
        self._call(self._lib.tetra_demod_process_resident, ptr(d_iq), int(n_samples), ptr(d_bits), int(bits_stride_), ptr(d_n_bits), ptr(d_sym))

    def process_device(self, d_iq, n_samples, d_bits, bits_stride_, d_n_bits, d_sym=None, stream=None):
        """Device path: arguments are objects with .data_ptr() (torch tensors on this GPU) or ints."""
        self._call(self._lib.tetra_demod_process_device, ptr(d_iq), int(n_samples), ptr(d_bits), int(bits_stride_), ptr(d_n_bits), ptr(d_sym),
                   stream_ptr(stream))

    # --- PI4DQPSK::reset and the setters -----------------------------------------------------------
    def reset(self, channel=-1):
        self._call(self._lib.tetra_demod_reset, channel)

    def set_param(self, name, value):
        self._call(self._lib.tetra_demod_set_param, PARAMS[name], float(value))

    def set_rrc_params(self, rrc_tap_count, rrc_beta):
        """PI4DQPSK::setRRCParams: both in one re-design."""
        self._call(self._lib.tetra_demod_set_rrc_params, int(rrc_tap_count), float(rrc_beta))

    def set_tables(self, rrc_taps=None, bandedge_taps=None, interp_bank=None):
        """tetra_demod_set_tables: FIR::setTaps with caller-designed tables (rrc [n]; band-edge [2][n_be] = re, im of the lower
        filter; bank [128][8]); None keeps a table."""
        r = None if rrc_taps is None else np.ascontiguousarray(rrc_taps, np.float32)
        b = None if bandedge_taps is None else np.ascontiguousarray(bandedge_taps, np.float32).reshape(2, -1)
        k = None if interp_bank is None else np.ascontiguousarray(interp_bank, np.float32).reshape(128, 8)
        self._call(self._lib.tetra_demod_set_tables, ptr(r), 0 if r is None else r.size, ptr(b), 0 if b is None else b.shape[1], ptr(k))

    def get_state(self, channel):
        st = ChannelState()
        self._call(self._lib.tetra_demod_get_state, channel, C.byref(st))
        return st

    def set_state(self, channel, st):
        self._call(self._lib.tetra_demod_set_state, channel, C.byref(st))

    def tables(self):
        nt, nbe = C.c_int(0), C.c_int(0)
        rrc = np.zeros(129, np.float32)          # TETRA_DEMOD_MAX_TAPS
        re = np.zeros(129, np.float32)
        im = np.zeros(129, np.float32)
        bank = np.zeros((128, 8), np.float32)
        self._call(self._lib.tetra_demod_get_tables, C.byref(nt), ptr(rrc), C.byref(nbe), ptr(re), ptr(im), ptr(bank))
        assert nbe.value == self._lib.tetra_demod_bandedge_tap_count(self._h)
        return dict(rrc=rrc[:nt.value].copy(), be_re=re[:nbe.value].copy(), be_im=im[:nbe.value].copy(), bank=bank)

    def read_rrc_out(self, n_samples):
        y = np.zeros((self.n_channels, n_samples), np.complex64)
        self._call(self._lib.tetra_demod_debug_read_rrc_out, ptr(y), n_samples)
        return y

    def selftest(self, in128):
        a = np.ascontiguousarray(in128, np.float32)
        assert a.shape == (128,)
        out = np.zeros(320, np.float32)
        self._call(self._lib.tetra_demod_debug_selftest, ptr(a), ptr(out))
        return out.reshape(5, 64)

    def mfma_selftest(self, a, b):
        """d = a . b on the matrix pipe (chained f32 MFMAs over ascending k from +0); a [M][K], b [K][M], M = 16 or 32."""
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        m, k = a.shape
        assert b.shape == (k, m)
        d = np.zeros((m, m), np.float32)
        self._call(self._lib.tetra_demod_debug_mfma_selftest, m, k, ptr(a), ptr(b), ptr(d))
        return d

    def quality(self):
        """(standarderr float32[C], sync bool[C]) -- DQPSKSymbolExtractor's public members per channel."""
        err = np.zeros(self.n_channels, np.float32)
        sync = np.zeros(self.n_channels, np.uint8)
        self._call(self._lib.tetra_demod_get_quality, ptr(err), ptr(sync))
        return err, sync.astype(bool)

    def constellation(self, first=0, count=None):
        """(blocks complex64[count][1024], n_blocks int32[count]) -- the last complete 1024-symbol block of the plugin's constellation
        tap per channel (src/main.cpp:85-89, :376-383) and the number of blocks completed; needs FLAG_CONSTELLATION."""
        count = self.n_channels - first if count is None else count
        blk = np.zeros((max(count, 0), CONSTELLATION_SYMBOLS), np.complex64)
        nb = np.zeros(max(count, 0), np.int32)
        self._call(self._lib.tetra_demod_get_constellation, first, count, ptr(blk), ptr(nb))
        return blk, nb

    def kernel_ms_history(self, n):
        """GPU ms of the n most recent process calls' launches, oldest first (HIP events on each call's stream)."""
        ms = np.zeros(n, np.float32)
        self._call(self._lib.tetra_demod_kernel_ms_history, n, ptr(ms))
        return ms

    def last_kernel_ms(self):
        a = C.c_float(0)
        self._call(self._lib.tetra_demod_last_kernel_ms, C.byref(a))
        return a.value
