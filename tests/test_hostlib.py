"""oracle/hostlib.py, the builder of the host-side checker libraries: current by content, not by file time."""
import ctypes as C
import os
import subprocess
import sys
import time

from oracle import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "int answer(void) {\n    return %d;\n}\n"
# the compile command logs every run, so that a test can count the compilations
CMD = ["sh", "-c", 'echo compiled >> compiles.log && exec gcc -shared -fPIC -o "$0" f.c', hostlib.OUT]


def _compiles(d):
    log = d / "compiles.log"
    return len(log.read_text().split()) if log.exists() else 0


def _answer(path):
    # (a copy under a new name: the loader would hand back an already loaded library of the same path)
    fresh = "%s.%d.so" % (path, time.monotonic_ns())
    with open(path, "rb") as f, open(fresh, "wb") as g:
        g.write(f.read())
    L = C.CDLL(fresh)
    L.answer.restype, L.answer.argtypes = C.c_int, []
    return L.answer()


def test_current_by_content_not_by_file_time(tmp_path):
    src, out = tmp_path / "f.c", str(tmp_path / "libf.so")
    src.write_text(SRC % 1)
    assert hostlib.build(out, CMD, [str(src)]) == out
    hostlib.build(out, CMD, [str(src)])
    assert _compiles(tmp_path) == 1 and _answer(out) == 1                  # building twice compiles once
    src.write_text(SRC % 2)
    os.utime(src, (1000000, 1000000))                                       # new content, a time long before the library's
    hostlib.build(out, CMD, [str(src)])
    assert _compiles(tmp_path) == 2 and _answer(out) == 2
    os.utime(src, None)                                                     # touched, same content
    hostlib.build(out, CMD, [str(src)])
    assert _compiles(tmp_path) == 2
    hostlib.build(out, CMD[:2] + [CMD[2] + " -O1"] + CMD[3:], [str(src)])   # another command
    assert _compiles(tmp_path) == 3 and _answer(out) == 2
    hostlib.build(out, CMD, [str(src)], extra="another host")              # whatever else the caller says it depends on
    assert _compiles(tmp_path) == 4
    hostlib.build(out, CMD, [str(src)], extra="another host", force=True)
    assert _compiles(tmp_path) == 5
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]            # nothing half-built is left behind


def test_two_processes_at_once_both_get_a_loadable_library(tmp_path):
    (tmp_path / "f.c").write_text(SRC % 7)
    prog = ("import ctypes, sys; sys.path.insert(0, %r); from oracle import hostlib\n"
            "L = hostlib.load(hostlib.build(%r, %r, [%r]), {'answer': (ctypes.c_int, [])})\n"
            "sys.exit(0 if L.answer() == 7 else 1)\n" % (ROOT, str(tmp_path / "libf.so"), CMD, str(tmp_path / "f.c")))
    procs = [subprocess.Popen([sys.executable, "-c", prog]) for _ in range(2)]
    assert [p.wait() for p in procs] == [0, 0]
    assert _compiles(tmp_path) == 1                                         # the second one waited at the lock and found the result
