"""What the built librpt_hip.so says about kernels 41 and 48: six waves per SIMD are 80 vector registers, and the
point of the parking is that they are reached WITHOUT scratch.  Read from the code object's notes the way tools/kernel_code_diff.py
reads them (llvm-readelf --notes; no device), so that a change that brings the spills back fails here and not in a benchmark."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_code_diff                                         # noqa: E402

LIB = os.path.join(ROOT, "relativitypathtracer_amd", "librpt_hip.so")
KERNELS_H = os.path.join(ROOT, "relativitypathtracer_amd", "csrc", "rpt_kernels.hip.h")


def park_bytes():
    """RPT_PARK_SLOTS x 64 lanes x 4 B, the slots as csrc/rpt_kernels.hip.h defines them"""
    with open(KERNELS_H) as f:
        slots = re.search(r"^#define RPT_PARK_SLOTS (\d+)$", f.read(), re.M)
    assert slots, "RPT_PARK_SLOTS is not defined in rpt_kernels.hip.h"
    return int(slots.group(1)) * 64 * 4


def kernel_blocks(notes):
    """{kernel name: {key: value}} from the amdhsa.kernels list of a code object's notes: a block begins at an entry of that list (a line
    "  - .key: value" at the list's own indentation) and holds that kernel's scalar keys, whatever their order"""
    lines = notes.splitlines()
    start = next((i for i, ln in enumerate(lines) if ln.strip() == "amdhsa.kernels:"), None)
    if start is None:
        return {}
    out, cur, indent = {}, None, None
    for ln in lines[start + 1:]:
        m = re.match(r"^(\s*)- (\.\w+):\s*(.*)$", ln)
        if m and (indent is None or len(m.group(1)) == indent):
            indent = len(m.group(1))
            if cur and ".name" in cur:
                out[cur[".name"]] = cur
            cur = {m.group(2): m.group(3).strip()}
            continue
        if indent is not None and ln.strip() and len(ln) - len(ln.lstrip()) < indent:
            break                                   # the list has ended (amdhsa.target, amdhsa.version)
        m = re.match(r"^(\s*)(\.\w+):\s*(\S.*)$", ln)
        if cur is not None and m and len(m.group(1)) == indent + 2:
            cur[m.group(2)] = m.group(3).strip()
    if cur and ".name" in cur:
        out[cur[".name"]] = cur
    return out


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kernel_code_diff.READELF):
        pytest.skip("llvm-readelf is not installed")
    assert os.path.exists(LIB), "librpt_hip.so is not built (__graft_entry__.build())"
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, code in enumerate(kernel_code_diff.code_objects(LIB)):
            path = os.path.join(tmp, f"co{k}.elf")
            with open(path, "wb") as f:
                f.write(code)
            notes = subprocess.run([kernel_code_diff.READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
            for name, k in kernel_blocks(notes).items():
                out[name] = dict(lds=int(k[".group_segment_fixed_size"]), scratch=int(k[".private_segment_fixed_size"]), vgprs=int(k[".vgpr_count"]))
    assert out, "no kernel metadata found in librpt_hip.so"
    return out


def _one(kernels, symbol):
    names = [n for n in kernels if re.search(rf"\d+{symbol}E", n)]
    assert len(names) == 1, f"{symbol}: {names}"
    return kernels[names[0]]


@pytest.mark.parametrize("symbol", ["rpt_render_kernel_ballot_w5", "rpt_render_kernel_ballot_ieee_w5"])
def test_six_waves_without_scratch(kernels, symbol):
    k = _one(kernels, symbol)
    print(symbol, k)
    assert k["scratch"] == 0, f"{symbol}: {k['scratch']} B of scratch per lane"
    assert k["vgprs"] <= 80, f"{symbol}: {k['vgprs']} vector registers do not fit six waves per SIMD"
    assert k["lds"] == park_bytes()
    assert 24 * k["lds"] <= 160 * 1024, "24 one-wave workgroups per CU: the LDS must not become the limit"


@pytest.mark.parametrize("symbol", ["rpt_render_kernel_ballot_first_w5", "rpt_render_kernel_analytic_w8", "rpt_render_kernel_unculled_w5"])
def test_kernels_without_the_flag_use_no_lds(kernels, symbol):
    assert _one(kernels, symbol)["lds"] == 0
