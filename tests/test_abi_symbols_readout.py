"""The readout calls (include/rpt.h, include/rpt_scene.h; DESIGN.md "Readout pass") are declared, exported by the two libraries and bound by
_ffi.py with their argument types, and rpt_readout has one layout in the header (as a C compiler lays it out) and in _ffi.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_readouts", "rpt_render_readouts", "rpt_render_readouts_async", "rpt_last_readout_pixels")


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_render_librarys_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert _declares("rpt.h", n), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_readouts.argtypes == [C.c_void_p, C.POINTER(_ffi.Readout), C.c_int]
    assert bound.rpt_render_readouts.argtypes == [C.c_void_p]
    assert bound.rpt_render_readouts_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_readout_pixels.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_scene_librarys_call_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    assert _declares("rpt_scene.h", "rpt_scene_get_readouts"), "include/rpt_scene.h does not declare rpt_scene_get_readouts"
    lib = _ffi.scene_lib()
    assert lib.rpt_scene_get_readouts.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    assert lib.rpt_scene_get_readouts.restype == C.c_int


def test_the_record_has_one_layout_in_the_header_and_in_python(tmp_path):
    from relativitypathtracer_amd import _ffi
    fields = ["rate", "offset", "u0", "v0", "u1", "v1", "digits", "decimals", "on_rgba", "off_rgba"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_readout));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_readout, {f}));\n' for f in fields) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Readout) == 36
    assert got[1:] == [getattr(_ffi.Readout, f).offset for f in fields]


def test_the_python_layer_has_the_feature():
    from relativitypathtracer_amd import Scene, events, worldline
    from relativitypathtracer_amd.renderer import Renderer
    assert callable(Renderer.set_readouts) and callable(Renderer.render_readouts) and callable(Renderer.last_readout_pixels)
    assert callable(Scene.readouts) and callable(events.readout) and callable(events.readout_settings) and callable(worldline.Worldline.clock_offsets)
