"""The one builder of the host-side checker libraries (the CPU oracle's, tests/emul's kernel emulations).  TEST INFRASTRUCTURE ONLY.

A library is current exactly when the key file next to it holds the sha256 over its dependencies' names and contents plus the
compile command -- file times say nothing after a checkout or a copy to another machine.  Otherwise it is rebuilt under a lock
file (ranks and pytest processes start together: one builds, the others find the result) and appears atomically (compiled next
to its final name, then renamed), the discipline of the product's build.py."""
import ctypes
import fcntl
import hashlib
import os
import subprocess

OUT = "{out}"      # stands for the output file in a compile command


def content_key(cmd, deps, extra=""):
    hsh = hashlib.sha256()
    for d in deps:
        with open(d, "rb") as f:
            hsh.update(os.path.basename(d).encode() + b"\0" + f.read() + b"\0")
    hsh.update("\0".join(cmd).encode() + b"\0" + extra.encode())
    return hsh.hexdigest()


def build(out, cmd, deps, extra="", force=False):
    """Make the library `out` current and return its path.  cmd: the compile command as a list, run in out's directory (so it can name
    its files relative to it and the key does not depend on where the tree lies), with OUT where the output file goes.  deps: every
    file the result depends on.  extra: anything else it depends on (e.g. the host's instruction set for -march=native)."""
    key = content_key(cmd, deps, extra)

    def current():
        try:
            with open(out + ".key") as f:
                return f.read() == key and os.path.exists(out)
        except OSError:
            return False

    if not force and current():
        return out
    with open(out + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or not current():
                tmp = "%s.tmp.%d" % (out, os.getpid())
                try:
                    subprocess.run([a.replace(OUT, os.path.basename(tmp)) for a in cmd], cwd=os.path.dirname(out), check=True,
                                   stdout=subprocess.DEVNULL)
                    if os.path.exists(out + ".key"):   # no key while the library changes: a key on disk always describes the
                        os.remove(out + ".key")        # library beside it
                    os.replace(tmp, out)
                    with open(tmp, "w") as f:
                        f.write(key)
                    os.replace(tmp, out + ".key")
                finally:
                    if os.path.exists(tmp):
                        os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return out


def load(path, signatures):
    """CDLL(path) with the table {name: (restype, [argtypes])} applied; a name the library lacks raises here."""
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in signatures.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    return L
