"""The ballistic-pass calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their
argument types, and rpt_ballistic has one layout — 48 bytes — in the header (as a C compiler lays it out), in _ffi.py and in ballistics.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_ballistics", "rpt_set_ballistic_options", "rpt_set_ballistic_temperatures", "rpt_render_ballistics", "rpt_render_ballistics_async",
         "rpt_last_ballistics", "rpt_set_ballistics_measurement", "rpt_last_ballistics_ms")


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_eight_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert _declares("rpt.h", n), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_ballistics.argtypes == [C.c_void_p, C.POINTER(_ffi.Ballistic), C.c_int]
    assert bound.rpt_set_ballistic_options.argtypes == [C.c_void_p, C.c_int, C.c_float]
    assert bound.rpt_set_ballistic_temperatures.argtypes == [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    assert bound.rpt_render_ballistics.argtypes == [C.c_void_p]
    assert bound.rpt_render_ballistics_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_ballistics.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert bound.rpt_set_ballistics_measurement.argtypes == [C.c_void_p, C.c_int]
    assert bound.rpt_last_ballistics_ms.argtypes == [C.c_void_p, C.POINTER(C.c_float)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_record_is_48_bytes_everywhere(tmp_path):
    from relativitypathtracer_amd import _ffi, ballistics
    fields = ["pos", "object", "rgb", "t0", "u", "t1"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_ballistic));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_ballistic, {f}));\n' for f in fields)
                   + '    printf(" %d\\n", RPT_PARTICLES_INVERSE_SQUARE);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Ballistic) == ballistics.BALLISTIC_DTYPE.itemsize == 48
    assert got[1:7] == [getattr(_ffi.Ballistic, f).offset for f in fields] == [ballistics.BALLISTIC_DTYPE.fields[f][1] for f in fields] == [0, 12, 16, 28, 32, 44]
    assert got[7] == ballistics.INVERSE_SQUARE == 1


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import ballistics, renderer
    R = renderer.Renderer
    assert all(callable(getattr(R, n)) for n in ("set_ballistics", "set_ballistic_options", "set_ballistic_temperatures", "render_ballistics", "last_ballistics"))
    assert list(inspect.signature(R.set_ballistics).parameters)[1:] == ["ballistics", "temperatures"]
    assert list(inspect.signature(R.set_ballistic_options).parameters)[1:] == ["inverse_square", "depth_bias"]
    assert {"ballistics", "ballistic_options", "ballistic_temperatures"} <= set(inspect.signature(renderer.render_scene).parameters)
    assert all(callable(getattr(ballistics, n)) for n in ("from_arrays", "jet", "shell", "save", "load", "project", "apparent_velocity"))
    assert list(inspect.signature(ballistics.from_arrays).parameters) == ["pos", "object", "rgb", "beta", "u", "t0", "t1", "epoch"]
