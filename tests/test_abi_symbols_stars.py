"""The star-field calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their
argument types, and rpt_star has one layout — 32 bytes — in the header (as a C compiler lays it out), in _ffi.py and in stars.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_stars", "rpt_render_stars", "rpt_render_stars_async", "rpt_last_stars")


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_four_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert _declares("rpt.h", n), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_stars.argtypes == [C.c_void_p, C.POINTER(_ffi.Star), C.c_int]
    assert bound.rpt_render_stars.argtypes == [C.c_void_p]
    assert bound.rpt_render_stars_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_stars.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_record_is_32_bytes_everywhere(tmp_path):
    from relativitypathtracer_amd import _ffi, stars
    fields = ["dir", "rgb", "_pad"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_star));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_star, {f}));\n' for f in fields) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Star) == stars.STAR_DTYPE.itemsize == 32
    assert got[1:] == [getattr(_ffi.Star, f).offset for f in fields] == [stars.STAR_DTYPE.fields[f][1] for f in fields]


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import renderer, stars
    R = renderer.Renderer
    assert callable(R.set_stars) and callable(R.render_stars) and callable(R.last_stars)
    assert "stars" in inspect.signature(renderer.render_scene).parameters
    assert all(callable(getattr(stars, n)) for n in ("random_catalogue", "from_arrays", "save", "load", "project"))
