"""Two builds of the library compared kernel by kernel, without a GPU: every gfx950 code object of both files' offload bundles is
disassembled (llvm-objdump -d, raw bytes and addresses dropped, branch targets reduced to "<+>") and split by symbol; the kernels'
register / LDS / scratch figures come from the code objects' metadata notes.

    python profiles/compare_device_code.py <parent's libtetra_demod_hip.so> <this build's>

Prints the symbols of the first file that are missing from or differ in the second (text or figures), and the second file's new
symbols with their figures; exit status 1 if any symbol of the first is missing or differs."""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def llvm(tool):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for d in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, tool)):
            return os.path.join(d, tool)
    return tool


def code_objects(lib, out):
    """the gfx950 entries of every bundle in the library's .hip_fatbin section -> files"""
    fat = os.path.join(out, "fat.bin")
    subprocess.run([llvm("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(out, "copy.so")], check=True)
    blob = open(fat, "rb").read()
    files, at = [], 0
    while True:
        at = blob.find(MAGIC, at)
        if at < 0:
            return files
        (num,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(num):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                files.append(os.path.join(out, "co%d.elf" % len(files)))
                open(files[-1], "wb").write(blob[at + off:at + off + size])
        at += len(MAGIC)


def symbols(lib):
    """-> ({symbol: [instruction text]}, {kernel: figures})"""
    text, figures = {}, {}
    with tempfile.TemporaryDirectory() as out:
        for f in code_objects(lib, out):
            dis = subprocess.run([llvm("llvm-objdump"), "-d", "--no-show-raw-insn", f], capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = m.group(1)
                    text[cur] = []
                elif cur is not None and line.strip():
                    line = re.sub(r"^\s*[0-9a-f]+:\s*", "", re.sub(r"//.*$", "", line))
                    text[cur].append(re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<+>", line).strip())
            notes = subprocess.run([llvm("llvm-readelf"), "--notes", f], capture_output=True, text=True, check=True).stdout
            for blk in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name:
                    get = lambda k: int((re.search(r"\.%s:\s+(\d+)" % k, blk) or [0, -1])[1])
                    figures[name.group(1)] = dict(vgpr=get("vgpr_count"), sgpr=get("sgpr_count"), lds=get("group_segment_fixed_size"),
                                                  scratch=get("private_segment_fixed_size"), workgroup=get("max_flat_workgroup_size"))
    return text, figures


def main():
    (a, fa), (b, fb) = symbols(sys.argv[1]), symbols(sys.argv[2])
    missing = sorted(s for s in a if s not in b)
    differ = sorted(s for s in a if s in b and a[s] != b[s])
    figures = sorted(s for s in fa if s in fb and fa[s] != fb[s])
    print("symbols: %d in the first file, %d in the second; missing %d, text differs %d, figures differ %d" % (len(a), len(b), len(missing), len(differ), len(figures)))
    for title, names in (("missing", missing), ("text differs", differ), ("figures differ", figures)):
        for s in names:
            print("  %s: %s" % (title, s))
    for s in sorted(b):
        if s not in a:
            print("  new: %s %d lines %s" % (s, len(b[s]), fb.get(s, "")))
    sys.exit(1 if missing or differ or figures else 0)


if __name__ == "__main__":
    main()
