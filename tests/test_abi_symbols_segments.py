"""The segment-pass calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their
argument types, rpt_segment has one layout — 48 bytes — in the header (as a C compiler lays it out), in _ffi.py and in segments.py, and
the two constants are the header's."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_segments", "rpt_set_segment_options", "rpt_render_segments", "rpt_render_segments_async", "rpt_last_segments",
         "rpt_set_segments_measurement", "rpt_last_segments_ms")


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_seven_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert _declares("rpt.h", n), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_segments.argtypes == [C.c_void_p, C.POINTER(_ffi.Segment), C.c_int]
    assert bound.rpt_set_segment_options.argtypes == [C.c_void_p, C.c_int, C.c_float, C.c_int]
    assert bound.rpt_render_segments.argtypes == [C.c_void_p]
    assert bound.rpt_render_segments_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_segments.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert bound.rpt_set_segments_measurement.argtypes == [C.c_void_p, C.c_int]
    assert bound.rpt_last_segments_ms.argtypes == [C.c_void_p, C.POINTER(C.c_float)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_record_is_48_bytes_everywhere_and_the_constants_are_the_headers(tmp_path):
    from relativitypathtracer_amd import _ffi, segments
    fields = ["a", "object", "b", "_pad0", "rgb", "_pad1"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_segment));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_segment, {f}));\n' for f in fields)
                   + '    printf(" %d %d\\n", RPT_SEGMENTS_INVERSE_SQUARE, RPT_SEGMENT_MAX_STEPS);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Segment) == segments.SEGMENT_DTYPE.itemsize == 48
    assert got[1:7] == [getattr(_ffi.Segment, f).offset for f in fields] == [segments.SEGMENT_DTYPE.fields[f][1] for f in fields] == [0, 12, 16, 28, 32, 44]
    assert got[7] == segments.INVERSE_SQUARE == 1
    assert got[8] == segments.MAX_STEPS == 1024


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import renderer, segments
    R = renderer.Renderer
    assert callable(R.set_segments) and callable(R.set_segment_options) and callable(R.render_segments) and callable(R.last_segments)
    assert list(inspect.signature(R.set_segment_options).parameters)[1:] == ["inverse_square", "depth_bias", "pieces"]
    assert inspect.signature(R.set_segment_options).parameters["pieces"].default == 16
    assert {"segments", "segment_options"} <= set(inspect.signature(renderer.render_scene).parameters)
    assert all(callable(getattr(segments, n)) for n in ("from_arrays", "polyline", "box_edges", "rod_lattice", "save", "load", "as_particles", "project"))
