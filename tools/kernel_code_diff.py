#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds of librpt_hip.so kernel by kernel (CPU only, no device needed).

Extracts every gfx950 code object from the offload bundles in each library's .hip_fatbin, disassembles it with llvm-objdump and
compares the instruction text of each kernel present in both (addresses, encodings and comments stripped).  Kernels only in the
second library are listed as new; the kernarg segment sizes from the code-object notes are printed for kernels whose size changed.
Exit status 1 if any kernel present in both differs.

usage: python tools/kernel_code_diff.py OLD.so NEW.so
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
OBJDUMP = os.path.join(ROCM, "llvm", "bin", "llvm-objdump")
READELF = os.path.join(ROCM, "llvm", "bin", "llvm-readelf")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib_path):
    data = open(lib_path, "rb").read()
    out = []
    pos = data.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", data, pos + 24)[0]
        p = pos + 32
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(data[pos + off:pos + off + size])
        pos = data.find(MAGIC, pos + 24)
    return out


def kernels(code, tmp):
    path = os.path.join(tmp, "co.elf")
    open(path, "wb").write(code)
    text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], capture_output=True, text=True, check=True).stdout
    ks, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+ )?<(.+)>:$", line.strip())
        if m:
            cur = m.group(2)
            ks[cur] = []
            continue
        if cur is None or not line.strip() or line.strip().startswith("Disassembly"):
            continue
        ins = re.sub(r"\s*//.*$", "", line).strip()
        if ins:
            ks[cur].append(re.sub(r"\s+", " ", ins))
    for body in ks.values():        # the padding behind a code object's last function is not that function's code
        while body and body[-1] in ("s_nop 0", "s_code_end"):
            body.pop()
    notes = subprocess.run([READELF, "--notes", path], capture_output=True, text=True).stdout
    sizes = {}
    for m in re.finditer(r"\.kernarg_segment_size:\s+(\d+).*?\.name:\s+(\S+)", notes, re.S):
        sizes[m.group(2)] = int(m.group(1))
    return ks, sizes


def collect(lib):
    ks, sizes = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib):
            k, s = kernels(co, tmp)
            ks.update(k)
            sizes.update(s)
    return ks, sizes


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, old_sizes = collect(sys.argv[1])
    new, new_sizes = collect(sys.argv[2])
    same = differ = 0
    for name in sorted(old):
        if name not in new:
            print(f"REMOVED  {name}")
            differ += 1
        elif old[name] != new[name]:
            print(f"DIFFERS  {name} ({len(old[name])} -> {len(new[name])} instructions)")
            differ += 1
        else:
            same += 1
    for name in sorted(set(new) - set(old)):
        print(f"NEW      {name} ({len(new[name])} instructions)")
    for name in sorted(set(old_sizes) & set(new_sizes)):
        if old_sizes[name] != new_sizes[name]:
            print(f"kernarg  {name}: {old_sizes[name]} -> {new_sizes[name]} B")
    print(f"{same} functions identical, {differ} differ or are missing")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
