"""The glare calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their argument
types, rpt_glare has one layout in the header (as a C compiler lays it out) and in _ffi.py, and the Python layer has the feature."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_glare", "rpt_glare_taps")


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_two_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert _declares("rpt.h", n), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_glare.argtypes == [C.c_void_p, C.POINTER(_ffi.Glare)]
    assert bound.rpt_glare_taps.argtypes == [C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_int)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_descriptor_has_one_layout(tmp_path):
    from relativitypathtracer_amd import _ffi, glare
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d %d\\n", sizeof(rpt_glare), offsetof(rpt_glare, layers), offsetof(rpt_glare, weight), offsetof(rpt_glare, sigma),\n'
                   '           RPT_GLARE_LAYERS_MAX, RPT_GLARE_RADIUS_MAX);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Glare) == 56
    assert got[1:4] == [_ffi.Glare.layers.offset, _ffi.Glare.weight.offset, _ffi.Glare.sigma.offset] == [0, 8, 32]
    assert got[4:] == [glare.LAYERS_MAX, glare.RADIUS_MAX] == [3, 32]


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import glare, renderer
    assert callable(renderer.Renderer.set_glare)
    assert list(inspect.signature(renderer.Renderer.set_glare).parameters)[1:] == ["layers"]
    assert "glare" in inspect.signature(renderer.render_scene).parameters
    assert list(inspect.signature(glare.taps).parameters) == ["sigma"]
    assert list(inspect.signature(glare.apply).parameters) == ["acc", "layers", "hit_mask", "wrap"]
    assert list(inspect.signature(glare.preset).parameters) == ["name"]
    for name in glare.PRESETS:
        assert sum(glare.weights(glare.preset(name))) == 65536
