"""The rocket-pass calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their
argument types, and rpt_rocket has one layout — 64 bytes — in the header (as a C compiler lays it out), in _ffi.py and in rockets.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_rockets", "rpt_set_rocket_options", "rpt_set_rocket_temperatures", "rpt_render_rockets", "rpt_render_rockets_async",
         "rpt_last_rockets", "rpt_set_rockets_measurement", "rpt_last_rockets_ms")


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
    assert bound.rpt_set_rockets.argtypes == [C.c_void_p, C.POINTER(_ffi.Rocket), C.c_int]
    assert bound.rpt_set_rocket_options.argtypes == [C.c_void_p, C.c_int, C.c_float]
    assert bound.rpt_set_rocket_temperatures.argtypes == [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    assert bound.rpt_render_rockets.argtypes == [C.c_void_p]
    assert bound.rpt_render_rockets_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_rockets.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert bound.rpt_set_rockets_measurement.argtypes == [C.c_void_p, C.c_int]
    assert bound.rpt_last_rockets_ms.argtypes == [C.c_void_p, C.POINTER(C.c_float)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_record_is_64_bytes_everywhere(tmp_path):
    from relativitypathtracer_amd import _ffi, rockets
    fields = ["pos", "object", "rgb", "t0", "u", "t1", "acc", "reserved"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_rocket));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_rocket, {f}));\n' for f in fields)
                   + '    printf(" %d\\n", RPT_PARTICLES_INVERSE_SQUARE);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Rocket) == rockets.ROCKET_DTYPE.itemsize == 64
    assert got[1:9] == [getattr(_ffi.Rocket, f).offset for f in fields] == [rockets.ROCKET_DTYPE.fields[f][1] for f in fields] == [0, 12, 16, 28, 32, 44, 48, 60]
    assert got[9] == rockets.INVERSE_SQUARE == 1


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import renderer, rockets
    R = renderer.Renderer
    assert all(callable(getattr(R, n)) for n in ("set_rockets", "set_rocket_options", "set_rocket_temperatures", "render_rockets", "last_rockets"))
    assert list(inspect.signature(R.set_rockets).parameters)[1:] == ["rockets", "temperatures"]
    assert list(inspect.signature(R.set_rocket_options).parameters)[1:] == ["inverse_square", "depth_bias"]
    assert list(inspect.signature(R.render_rockets).parameters)[1:] == ["async_"]
    assert {"rockets", "rocket_options", "rocket_temperatures"} <= set(inspect.signature(renderer.render_scene).parameters)
    assert all(callable(getattr(rockets, n)) for n in ("from_arrays", "from_ballistics", "launch", "fleet", "trip", "as_ballistics", "save", "load", "project",
                                                       "redshift_from_pad"))
    assert list(inspect.signature(rockets.from_arrays).parameters) == ["pos", "object", "rgb", "beta", "u", "acc", "t0", "t1", "epoch"]
    assert list(inspect.signature(rockets.launch).parameters) == ["object", "origin", "acc", "n_times", "rgb"]
    assert list(inspect.signature(rockets.fleet).parameters)[:4] == ["object", "positions", "acc", "rigid"]
    assert list(inspect.signature(rockets.trip).parameters) == ["object", "origin", "direction", "acc", "leg_proper_time", "rgb"]
