"""rpt_tile_bitmap_stage_host (include/rpt.h; csrc/rpt_tile_bitmap.hpp: one stage of the tile bitmap alone) is declared, exported by the
render library and bound by _ffi.py with its argument types."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_stage_call_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    assert _declares("rpt.h", "rpt_tile_bitmap_stage_host"), "include/rpt.h does not declare rpt_tile_bitmap_stage_host"
    assert hasattr(C.CDLL(_ffi.hip_lib_path()), "rpt_tile_bitmap_stage_host"), "librpt_hip.so does not export rpt_tile_bitmap_stage_host"
    assert "rpt_tile_bitmap_stage_host" in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_tile_bitmap_stage_host.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                                         C.c_size_t, C.POINTER(C.c_int)]
    assert bound.rpt_tile_bitmap_stage_host.restype == C.c_int


def test_the_rasterisation_hook_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    assert _declares("rpt.h", "rpt_tile_rasterise_host"), "include/rpt.h does not declare rpt_tile_rasterise_host"
    assert hasattr(C.CDLL(_ffi.hip_lib_path()), "rpt_tile_rasterise_host"), "librpt_hip.so does not export rpt_tile_rasterise_host"
    bound = _ffi.hip()
    assert bound.rpt_tile_rasterise_host.argtypes == [C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_float), C.c_void_p, C.c_size_t]
    assert bound.rpt_tile_rasterise_host.restype == C.c_int


def test_the_shared_state_call_is_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    assert _declares("rpt.h", "rpt_tile_bitmap_shared_state"), "include/rpt.h does not declare rpt_tile_bitmap_shared_state"
    assert hasattr(C.CDLL(_ffi.hip_lib_path()), "rpt_tile_bitmap_shared_state"), "librpt_hip.so does not export rpt_tile_bitmap_shared_state"
    bound = _ffi.hip()
    assert bound.rpt_tile_bitmap_shared_state.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert bound.rpt_tile_bitmap_shared_state.restype == C.c_int


def test_the_earlier_calls_keep_their_types():
    from relativitypathtracer_amd import _ffi
    bound = _ffi.hip()
    assert bound.rpt_tile_bitmap_host.argtypes == [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                   C.c_size_t, C.POINTER(C.c_int)]
    assert bound.rpt_tile_bitmap_state.argtypes == [C.c_void_p, C.POINTER(C.c_uint64), C.c_int, C.c_void_p, C.c_size_t]
