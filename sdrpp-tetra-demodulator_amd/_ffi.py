"""The one ctypes call layer under every *_binding module: pointer and stream conversion, the status check, and the application of a
module's signature table {name: (restype, [argtypes])} to the loaded library."""
import ctypes as C

# shorthands the signature tables are written in
vp, i32, u32, i64, u64, f64, size_t = C.c_void_p, C.c_int, C.c_uint32, C.c_int64, C.c_uint64, C.c_double, C.c_size_t
P = C.POINTER


class TetraDemodError(RuntimeError):
    def __init__(self, status, what, hip=0):
        self.status = status
        self.hip = hip
        msg = "%s failed: %d (%s)" % (what, status, _strerror(status))
        if hip:
            msg += " [hipError %d]" % hip
        super().__init__(msg)


def _strerror(status):
    try:
        from .binding import load_library
        return load_library(False).tetra_demod_strerror(status).decode()
    except Exception:  # pragma: no cover
        return "?"


def ptr(x):
    """An address for a c_void_p parameter: None stays None, an object with .data_ptr() (torch tensor) or a numpy array gives its
    data address, an int is passed through."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    return int(x)


def stream_ptr(s):
    """A torch stream or a raw hipStream_t (int) -> the raw handle; None = the null stream."""
    if s is None:
        return None
    return s.cuda_stream if hasattr(s, "cuda_stream") else int(s)


def check(rc, fn, hip=0):
    """Raise TetraDemodError for a non-zero status.  fn: the library function that returned it (named by its own __name__), or a text."""
    if rc:
        raise TetraDemodError(rc, getattr(fn, "__name__", fn), hip)


def call(fn, *args):
    """fn(*args) for a library function that returns a status; a non-zero one raises under the function's own name."""
    rc = fn(*args)
    if rc:
        raise TetraDemodError(rc, fn.__name__)


def declare(L, signatures, optional=()):
    """Apply a signature table to the library L.  Names in `optional` may be missing (a TETRA_DEMOD_LIB override can be an older
    experimental build); any other missing name raises here, at load, not at the first call."""
    for name, (restype, argtypes) in signatures.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if name in optional:
                continue
            raise RuntimeError("%s does not export %s" % (L._name, name))
        fn.restype, fn.argtypes = restype, argtypes
    return L
