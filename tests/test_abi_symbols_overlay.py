"""The overlay calls of include/rpt.h are declared, exported and bound with their argument types, and rpt_overlay_desc has one size in
the header (as a C compiler lays it out) and in _ffi.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_overlay", "rpt_render_overlay", "rpt_render_overlay_async", "rpt_last_overlay_pixels")


def test_overlay_symbols_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_overlay.argtypes == [C.c_void_p, C.POINTER(_ffi.OverlayDesc)]
    assert bound.rpt_render_overlay.argtypes == [C.c_void_p]
    assert bound.rpt_render_overlay_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_overlay_pixels.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]


def test_the_description_has_one_layout_in_the_header_and_in_python(tmp_path):
    from relativitypathtracer_amd import _ffi
    fields = ["layers", "delay_step", "clock_step", "lattice_step", "tint_t_max", "outline_rgba", "delay_rgba", "clock_rgba", "lattice_rgba", "tint_alpha"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_overlay_desc));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_overlay_desc, {f}));\n' for f in fields)
                   + '    printf(" %d %d %d %d %d\\n", RPT_OVERLAY_OUTLINES, RPT_OVERLAY_ISO_DELAY, RPT_OVERLAY_ISO_CLOCK, RPT_OVERLAY_LATTICE, RPT_OVERLAY_DELAY_TINT);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.OverlayDesc) == 48
    assert got[1:1 + len(fields)] == [getattr(_ffi.OverlayDesc, f).offset for f in fields]
    from relativitypathtracer_amd import events
    assert got[1 + len(fields):] == [events.OVERLAY_OUTLINES, events.OVERLAY_ISO_DELAY, events.OVERLAY_ISO_CLOCK, events.OVERLAY_LATTICE, events.OVERLAY_DELAY_TINT]
