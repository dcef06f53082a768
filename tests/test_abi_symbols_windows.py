"""The time-window calls (include/rpt.h, include/rpt_scene.h; DESIGN.md "Time windows") are declared, exported by the two libraries and
bound by _ffi.py with their argument types."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_render_librarys_call_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    assert _declares("rpt.h", "rpt_set_object_windows"), "include/rpt.h does not declare rpt_set_object_windows"
    assert hasattr(C.CDLL(_ffi.hip_lib_path()), "rpt_set_object_windows"), "librpt_hip.so does not export rpt_set_object_windows"
    assert "rpt_set_object_windows" in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_object_windows.argtypes == [C.c_void_p, C.c_void_p, C.c_int]
    assert bound.rpt_set_object_windows.restype == C.c_int


def test_the_scene_librarys_call_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    assert _declares("rpt_scene.h", "rpt_scene_get_windows"), "include/rpt_scene.h does not declare rpt_scene_get_windows"
    lib = _ffi.scene_lib()
    assert lib.rpt_scene_get_windows.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    assert lib.rpt_scene_get_windows.restype == C.c_int


def test_the_python_layer_has_the_feature():
    from relativitypathtracer_amd import Scene, worldline
    from relativitypathtracer_amd.renderer import Renderer
    assert callable(Renderer.set_object_windows) and callable(Scene.windows) and callable(worldline.piecewise)
