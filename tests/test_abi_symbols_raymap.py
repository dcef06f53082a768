"""The ray-map calls of include/rpt.h are declared, exported by librpt_hip.so and bound by _ffi.py with their argument types, and the
header's constants are the ones the Python layer uses."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_raymap", "rpt_raymap_fill")


def test_raymap_symbols_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_raymap.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    assert bound.rpt_raymap_fill.argtypes == [C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_void_p]
    assert bound.rpt_set_raymap.restype == bound.rpt_raymap_fill.restype == C.c_int


def test_the_constants_of_the_header_are_the_python_layers():
    from relativitypathtracer_amd import renderer
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define\s+(RPT_(?:PROJECTION|RAYMAP)_\w+)\s+(\d+)\s*$", header, flags=re.M)}
    assert defines["RPT_PROJECTION_RAYMAP"] == renderer.PROJECTIONS["raymap"] == 2
    assert defines["RPT_PROJECTION_PINHOLE"] == renderer.PROJECTIONS["pinhole"] and defines["RPT_PROJECTION_EQUIRECT"] == renderer.PROJECTIONS["equirect"]
    assert {"fisheye": defines["RPT_RAYMAP_FISHEYE"], "equisolid": defines["RPT_RAYMAP_FISHEYE_EQUISOLID"],
            "stereographic": defines["RPT_RAYMAP_STEREOGRAPHIC"], "cube_strip": defines["RPT_RAYMAP_CUBE_STRIP"]} == renderer.RAYMAP_KINDS
    assert len(set(renderer.RAYMAP_KINDS.values())) == 4
