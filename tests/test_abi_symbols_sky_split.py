"""rpt_last_sky_split (include/rpt.h) is declared, exported by the render library and bound by _ffi.py with its argument
types; the Python layer has the query; without a context the call answers "one launch" and four zeros (no device needed)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_query_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi, renderer
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpt.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rpt_last_sky_split\s*\(\s*const\s+rpt_ctx\s*\*\s*ctx\s*,\s*int\s+rect\[4\]\s*\)", code)
    assert hasattr(C.CDLL(_ffi.hip_lib_path()), "rpt_last_sky_split") and "rpt_last_sky_split" in _ffi.HIP_SYMBOLS
    bound = _ffi.hip().rpt_last_sky_split
    assert bound.argtypes == [C.c_void_p, C.POINTER(C.c_int)] and bound.restype == C.c_int
    rect = (C.c_int * 4)(7, 7, 7, 7)
    assert bound(None, rect) == 0 and list(rect) == [0, 0, 0, 0]
    assert bound(None, None) == 0
    assert callable(renderer.Renderer.last_sky_split)
