#!/usr/bin/env python3
"""The static record of a libmof_hip.so: every kernel of every gfx950 code object with the numeric fields of its metadata note, `bytes`,
the size of the kernel's symbol in .text, and `code`, a SHA-256 over the bytes of the kernel's symbol in .text followed by its 64-byte descriptor <name>.kd -- without the descriptor's
kernel_code_entry_byte_offset (bytes 16 .. 23), the distance from the descriptor to the entry, which moves whenever another kernel joins
or leaves the code object.

  tools/kernel_static.py LIB             one line per kernel, sorted by name
  tools/kernel_static.py compare A B [REGEX=REPL ...]
                                         whether each whole gfx950 code object is byte-identical (by position, and by content: a new
                                         translation unit shifts the positions behind it), then the names only in A, the names only
                                         in B, and the fields (code included) that changed

Reads metadata, the symbol table and the section headers (llvm-readelf --notes / --symbols / --section-headers on the unbundled code
objects) and slices the symbols' bytes out of the file: no disassembly, no instruction is looked at. `code` covers the kernel's own
symbol only: a change in a device function it calls (none is left un-inlined in this library) shows in the whole-object line alone.
"""
import hashlib
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


def code_hashes(co, sections, symbols):
    """{mangled name: sha256 hex of the symbol's bytes + its .kd descriptor, entry offset zeroed} from the text of llvm-readelf -S and -s
    of code object `co`."""
    sec = {}  # index -> (address, file offset)
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S+\s+(?:PROGBITS)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+[0-9a-f]+", sections, re.M):
        sec[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
    sym = {}  # name -> bytes
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+(?:FUNC|OBJECT)\s+\S+\s+\S+\s+(\d+)\s+(\S+)\s*$", symbols, re.M):
        addr, size, ndx, name = int(m.group(1), 16), int(m.group(2)), int(m.group(3)), m.group(4)
        if ndx in sec:
            off = sec[ndx][1] + addr - sec[ndx][0]
            sym[name] = co[off:off + size]
    return {n: (hashlib.sha256(b + sym[n + ".kd"][:16] + bytes(8) + sym[n + ".kd"][24:]).hexdigest(), len(b), hashlib.sha256(b).hexdigest())
            for n, b in sym.items() if n + ".kd" in sym}


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
            code = code_hashes(co, subprocess.check_output([readelf, "-S", "-W", path], text=True),
                               subprocess.check_output([readelf, "--symbols", "-W", path], text=True))
            for name, fields in kernels_of(subprocess.check_output([readelf, "--notes", path], text=True)).items():
                if name not in code:
                    sys.exit(f"{lib}: no symbol or no descriptor {name}.kd found for kernel {name} (llvm-readelf --symbols)")
                fields["code"], fields["code_bytes"], fields["text"] = code[name]
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
    return " ".join(f"{s} {fields.get(k, 0)}" for s, k in zip(SHORT, FIELDS)) + f" bytes {fields['code_bytes']} code {fields['code'][:16]}"


def main(argv):
    if len(argv) == 2:
        rec = record(argv[1])
        for name in sorted(rec):
            print(f"{name}: {row(rec[name])}")
        print(f"kernels: {len(rec)}")
        return 0
    if len(argv) >= 4 and argv[1] == "compare":
        # compare A B [REGEX=REPLACEMENT ...]: the kernel names of both sides rewritten first (a template that gained a defaulted
        # parameter names its old instantiations differently: 'kernel<(.*), false>=kernel<\\1>')
        for rule in argv[4:]:
            pat, _, repl = rule.partition("=")
            print(f"names rewritten: {pat} -> {repl}")
        ca, cb = [[hashlib.sha256(co).hexdigest() for co in code_objects(lib)] for lib in (argv[2], argv[3])]
        same = sum(x == y for x, y in zip(ca, cb))
        print(f"gfx950 code objects: A {len(ca)}, B {len(cb)}; byte-identical {same}" + ("" if len(ca) != len(cb) else f", differing {len(ca) - same}"))
        for i, (x, y) in enumerate(zip(ca, cb)):
            print(f"  code object {i}: {'identical' if x == y else f'DIFFERS {x[:16]} -> {y[:16]}'}")
        # (the linker places a translation unit's bundle where it likes: one more unit shifts the positions behind it, so also by content)
        gone, new = [x for x in ca if x not in cb], [y for y in cb if y not in ca]
        print(f"by content: {len(ca) - len(gone)} of A's {len(ca)} code objects are byte-identical in B; only in A {[x[:16] for x in gone]}, "
              f"only in B {[y[:16] for y in new]}")
        a, b = record(argv[2]), record(argv[3])
        for rule in argv[4:]:
            pat, _, repl = rule.partition("=")
            a, b = ({re.sub(pat, repl, n): f for n, f in r.items()} for r in (a, b))
        only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        print(f"kernels: A {len(a)}, B {len(b)}; library {os.path.getsize(argv[2])} -> {os.path.getsize(argv[3])} bytes")
        print(f"only in A: {only_a}")
        print(f"only in B: {only_b}")
        changed = 0
        for name in sorted(set(a) & set(b)):
            diff = [f"{s} {a[name].get(k, 0)} -> {b[name].get(k, 0)}" for s, k in zip(SHORT, FIELDS) if a[name].get(k, 0) != b[name].get(k, 0)]
            if a[name]["code"] != b[name]["code"]:
                # (same instruction bytes: only the descriptor differs -- e.g. kernarg_size after a member was appended to an argument struct)
                diff.append(f"code {a[name]['code'][:16]} -> {b[name]['code'][:16]}" + (" (descriptor only: .text bytes identical)" if a[name]["text"] == b[name]["text"] else ""))
            if diff:
                changed += 1
                print(f"{name}: {', '.join(diff)}")
        print(f"changed in any field: {changed}")
        return 1 if (only_a or only_b or changed) else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv))
