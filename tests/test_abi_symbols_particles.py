"""The particle-pass calls (include/rpt.h) are declared, exported by the render library and bound by _ffi.py with their
argument types, and rpt_particle has one layout — 32 bytes — in the header (as a C compiler lays it out), in _ffi.py and in particles.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rpt_set_particles", "rpt_set_particle_options", "rpt_render_particles", "rpt_render_particles_async", "rpt_last_particles")


def _declares(header, name):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return re.search(r"\bint\s+" + name + r"\s*\(", code) is not None


def test_the_five_calls_are_declared_exported_and_bound():
    from relativitypathtracer_amd import _ffi
    lib = C.CDLL(_ffi.hip_lib_path())
    for n in NAMES:
        assert _declares("rpt.h", n), f"include/rpt.h does not declare {n}"
        assert hasattr(lib, n), f"librpt_hip.so does not export {n}"
        assert n in _ffi.HIP_SYMBOLS
    bound = _ffi.hip()
    assert bound.rpt_set_particles.argtypes == [C.c_void_p, C.POINTER(_ffi.Particle), C.c_int]
    assert bound.rpt_set_particle_options.argtypes == [C.c_void_p, C.c_int, C.c_float]
    assert bound.rpt_render_particles.argtypes == [C.c_void_p]
    assert bound.rpt_render_particles_async.argtypes == [C.c_void_p]
    assert bound.rpt_last_particles.argtypes == [C.c_void_p, C.POINTER(C.c_uint64)]
    assert all(getattr(bound, n).restype == C.c_int for n in NAMES)


def test_the_record_is_32_bytes_everywhere(tmp_path):
    from relativitypathtracer_amd import _ffi, particles
    fields = ["pos", "object", "rgb", "_pad"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rpt.h"\nint main(void) {\n    printf("%zu", sizeof(rpt_particle));\n'
                   + "".join(f'    printf(" %zu", offsetof(rpt_particle, {f}));\n' for f in fields)
                   + '    printf(" %d\\n", RPT_PARTICLES_INVERSE_SQUARE);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert got[0] == C.sizeof(_ffi.Particle) == particles.PARTICLE_DTYPE.itemsize == 32
    assert got[1:5] == [getattr(_ffi.Particle, f).offset for f in fields] == [particles.PARTICLE_DTYPE.fields[f][1] for f in fields] == [0, 12, 16, 28]
    assert got[5] == particles.INVERSE_SQUARE == 1


def test_the_python_layer_has_the_feature():
    import inspect
    from relativitypathtracer_amd import particles, renderer
    R = renderer.Renderer
    assert callable(R.set_particles) and callable(R.set_particle_options) and callable(R.render_particles) and callable(R.last_particles)
    assert list(inspect.signature(R.set_particle_options).parameters)[1:] == ["inverse_square", "depth_bias"]
    assert {"particles", "particle_options"} <= set(inspect.signature(renderer.render_scene).parameters)
    assert all(callable(getattr(particles, n)) for n in ("from_arrays", "lattice", "at_events", "save", "load", "project"))
