"""The adaptive anti-aliasing calls of include/rpt.h are exported, bound with their argument types, and named in the header's list."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_adaptive_aa", "rpt_last_aa_refined", "rpt_last_aa_variant")


def test_adaptive_aa_symbols_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    header = open(os.path.join(ROOT, "include", "rpt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_adaptive_aa.argtypes == [C.c_void_p, C.c_int, C.c_int]
    assert bound.rpt_last_aa_refined.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert bound.rpt_last_aa_variant.argtypes == [C.c_void_p]
