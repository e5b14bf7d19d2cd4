#!/usr/bin/env python3
"""The static record of a libmof_hip.so: every kernel of every gfx950 code object with the numeric fields of its metadata note.

  tools/kernel_static.py LIB             one line per kernel, sorted by name
  tools/kernel_static.py compare A B     the names only in A, the names only in B, and the fields that changed

Reads metadata only (llvm-readelf --notes on the unbundled code objects): no disassembly, no instruction is looked at.
"""
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count",
          ".group_segment_fixed_size")
SHORT = ("vgpr", "agpr", "sgpr", "scratch", "spill_v", "spill_s", "lds")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def tool(name):
    for d in [os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")] + os.environ.get("PATH", "").split(os.pathsep):
        if os.path.isfile(os.path.join(d, name)):
            return os.path.join(d, name)
    return None


def code_objects(lib, arch="gfx950"):
    """The code objects for `arch` of every offload bundle in the file (one bundle per translation unit)."""
    blob = open(lib, "rb").read()
    for m in re.finditer(MAGIC, blob):
        base = m.start()
        (count,) = struct.unpack_from("<Q", blob, base + len(MAGIC))
        pos = base + len(MAGIC) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", blob, pos)
            ident = blob[pos + 24:pos + 24 + idlen].decode()
            pos += 24 + idlen
            if size and ident.endswith(arch):
                yield blob[base + off:base + off + size]


def kernels_of(notes):
    """{mangled name: {field: int}} from the text of llvm-readelf --notes (the amdhsa.kernels list of the metadata note)."""
    out, cur, inside = {}, None, False
    for line in notes.splitlines():
        if not line.startswith(" "):
            inside = line.startswith("amdhsa.kernels:")
            continue
        if not inside:
            continue
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s*(\S*)\s*$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if m.group(2) == ".name":
            out[m.group(3)] = cur
        elif m.group(2) in FIELDS:
            cur[m.group(2)] = int(m.group(3))
    return out


def record(lib):
    readelf = tool("llvm-readelf")
    if not readelf:
        sys.exit("llvm-readelf not found (ROCM_PATH/llvm/bin or PATH)")
    rec = {}
    with tempfile.TemporaryDirectory() as tmp:
        for i, co in enumerate(code_objects(lib)):
            path = os.path.join(tmp, f"co{i}.elf")
            with open(path, "wb") as f:
                f.write(co)
            for name, fields in kernels_of(subprocess.check_output([readelf, "--notes", path], text=True)).items():
                while name in rec:  # (kernels of unnamed namespaces in two translation units may share a name)
                    name += "'"
                rec[name] = fields
    filt = tool("llvm-cxxfilt") or shutil.which("c++filt")
    if filt and rec:
        names = sorted(rec)
        plain = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        if len(plain) == len(names):
            rec = {p.replace("(anonymous namespace)::", "").replace("mof::", ""): rec[n] for n, p in zip(names, plain)}
    return rec


def row(fields):
    return " ".join(f"{s} {fields.get(k, 0)}" for s, k in zip(SHORT, FIELDS))


def main(argv):
    if len(argv) == 2:
        rec = record(argv[1])
        for name in sorted(rec):
            print(f"{name}: {row(rec[name])}")
        print(f"kernels: {len(rec)}")
        return 0
    if len(argv) == 4 and argv[1] == "compare":
        a, b = record(argv[2]), record(argv[3])
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        print(f"kernels: A {len(a)}, B {len(b)}; library {os.path.getsize(argv[2])} -> {os.path.getsize(argv[3])} bytes")
        print(f"only in A: {only_a}")
        print(f"only in B: {only_b}")
        changed = 0
        for name in sorted(set(a) & set(b)):
            diff = [f"{s} {a[name].get(k, 0)} -> {b[name].get(k, 0)}" for s, k in zip(SHORT, FIELDS) if a[name].get(k, 0) != b[name].get(k, 0)]
            if diff:
                changed += 1
                print(f"{name}: {', '.join(diff)}")
        print(f"changed in any field: {changed}")
        return 1 if (only_a or only_b or changed) else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
