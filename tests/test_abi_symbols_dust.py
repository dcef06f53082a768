"""The lit-particle calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their
argument types; the Python layer has the methods, the render_scene keyword and the model helpers; and rpt_set_particle_options still takes
its three arguments — the lighting is a setter of its own, not a fourth argument or a new bit of that call."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_particle_lighting", "rpt_last_particle_lighting")


def _code(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_the_two_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    code = _code("rpt.h")
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_particle_lighting.argtypes == [C.c_void_p, C.c_int]
    assert bound.rpt_last_particle_lighting.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_flags_have_their_values_in_the_header_and_in_particles_py(tmp_path):
    from relativitypathtracer_amd import particles
    src = tmp_path / "flags.c"
    src.write_text('#include <stdio.h>\n#include "rpt.h"\nint main(void) {\n'
                   '    printf("%d %d %d %d\\n", RPT_PARTICLES_LIT, RPT_PARTICLES_SHADOWED, RPT_PARTICLES_AMBIENT, RPT_PARTICLES_INVERSE_SQUARE);\n    return 0;\n}\n')
    exe = tmp_path / "flags"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [particles.LIT, particles.SHADOWED, particles.AMBIENT, particles.INVERSE_SQUARE] == [1, 2, 4, 1]


def test_rpt_set_particle_options_still_has_its_three_arguments():
    from relativitypathtracer_amd import _ffi
    m = re.search(r"\bint\s+rpt_set_particle_options\s*\(([^)]*)\)", _code("rpt.h"))
    assert m and [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["ctx", "flags", "depth_bias"]
    assert _ffi.hip().rpt_set_particle_options.argtypes == [C.c_void_p, C.c_int, C.c_float]


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import particles, renderer
    R = renderer.Renderer
    assert list(inspect.signature(R.set_particle_lighting).parameters)[1:] == ["lit", "shadows", "ambient"]
    assert all(p.default is False for p in list(inspect.signature(R.set_particle_lighting).parameters.values())[1:])
    assert callable(R.last_particle_lighting)
    assert list(inspect.signature(R.set_particle_options).parameters)[1:] == ["inverse_square", "depth_bias"]
    assert "particle_lighting" in inspect.signature(renderer.render_scene).parameters
    assert list(inspect.signature(particles.illuminate).parameters) == ["particles", "objects", "interval", "doppler", "ambient", "flags", "windows"]
    assert list(inspect.signature(particles.dust).parameters) == ["object", "lo", "hi", "count", "rgb", "seed"]
