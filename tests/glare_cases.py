"""The layer sets and sizes of the glare tests and the ctypes face of tests/native/glare_oracle.c — TEST INFRASTRUCTURE shared by
tests/test_glare_model.py (no GPU: glare.apply against the C stage, the taps against float64) and tests/test_gpu_glare.py (the five
passes with glare on against the C restatement of the passes with rules G2-G6 behind them).

glare_oracle.c is built once per pass on top of that pass's own restatement (KINDS), so every library here also has the plain pass
functions, bound as the pass's own cases module binds them: sc.oracle_pass, pc.oracle_pass, gc.oracle_pass, dc.oracle_pass,
bc.oracle_pass, rc.oracle_pass and thermal_cases' two take these libraries too.  `glared` runs one of them and puts the stage behind its
accumulator."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
import oracle_ffi
import particles_cases as pc
import stars_cases as sc
from relativitypathtracer_amd import _ffi, glare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "glare_oracle.c")
KINDS = ("stars", "segments", "dust", "ballistics", "rockets")     # "segments" has the plain particle pass, "ballistics" the thermal one

# the model's sizes (no GPU): (W, H, wrap, sigma of the widest layer).  300 x 70: two row segments of 256, the second partial, taller
# than 2 R + 1; 40 x 24 with R = 32: the support leaves the frame on both sides at once; 24 x 16 wrapped with R = 32: the modulo is
# taken more than once
MODEL_SIZES = [(300, 70, False), (40, 24, False), (24, 16, True)]
SIZES = [(300, 70), (40, 24)]               # the GPU tests'
LAYER_SETS = {"narrow": [(0.4, 0.7)],
              "three": [(0.3, 1.0), (0.2, 4.0), (0.1, 32.0 / 3.0)],      # the widest there is: R = 32
              "no core": [(0.5, 0.5), (0.5, 2.5)]}                       # w_0 = 0
SIGMAS = [0.5, 0.7, 1.0, 2.5, 6.0, 32.0 / 3.0]

P, I = C.c_void_p, C.c_int
_PARTICLE_PASS = [C.POINTER(pc.ParticlesView), P, I, P, P, I, P, P, P]
_BOUND = {
    "stars": {"rpt_stars_oracle_pass": [C.POINTER(sc.StarsView), P, I, P, P, P],
              "rpt_thermal_oracle_stars_pass": [C.POINTER(sc.StarsView), P, P, I, P, P, P]},
    "segments": {"rpt_particles_oracle_pass": _PARTICLE_PASS,
                 "rpt_segments_oracle_pass": [C.POINTER(pc.ParticlesView), P, I, P, P, I, I] + [P] * 6},
    "dust": {"rpt_dust_oracle_pass": [C.POINTER(oracle_ffi.OracleArgs), C.POINTER(pc.ParticlesView), I, P, P, I, P, P, P]},
    "ballistics": {"rpt_ballistics_oracle_pass": _PARTICLE_PASS,
                   "rpt_thermal_oracle_particles_pass": [C.POINTER(pc.ParticlesView), P, I, P, P, P, I, P, P, P]},
    "rockets": {"rpt_rockets_oracle_pass": _PARTICLE_PASS},
}


def build_library(directory, kind) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/glare_oracle.c")
    so = os.path.join(str(directory), f"libglare_{kind}_oracle.so")
    p = subprocess.run(["gcc", *eo.CFLAGS, f"-DGLARE_{kind.upper()}", "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    for name, args in _BOUND[kind].items():
        f = getattr(lib, name)
        f.restype, f.argtypes = I, args
    lib.rpt_glare_oracle_arm.restype, lib.rpt_glare_oracle_arm.argtypes = I, [C.c_size_t]
    lib.rpt_glare_oracle_captured.restype, lib.rpt_glare_oracle_captured.argtypes = I, [P, C.c_size_t]
    lib.rpt_glare_oracle_stage.restype, lib.rpt_glare_oracle_stage.argtypes = I, [P, I, I, I, P, I, P, P, P, P]
    lib.rpt_glare_oracle_resolve.restype, lib.rpt_glare_oracle_resolve.argtypes = I, [P, I, I, P, P, P]
    return lib


def integers(layers):
    """Rules G0 and G1 for the C stage: (weights uint32[4], taps uint32[len][65], radius int32[3]), the taps from rpt_glare_taps."""
    w = np.zeros(4, dtype=np.uint32)
    w[:len(layers) + 1] = glare.weights(layers)
    taps = np.zeros((max(len(layers), 1), 65), dtype=np.uint32)
    radius = np.zeros(3, dtype=np.int32)
    for k, (_, sigma) in enumerate(layers):
        t, R = glare.taps(sigma)
        taps[k, 32 - R:32 + R + 1] = t
        radius[k] = R
    return w, taps, radius


def oracle_stage(lib, acc, layers, records=None, wrap=False):
    """Rules G2-G5 in C on an (H, W, 3) uint64 accumulator: S, (H, W, 3) uint64.  records: the star pass's mask, (H, W) event records."""
    a = np.ascontiguousarray(acc, dtype=np.uint64)
    H, W, _ = a.shape
    w, taps, radius = integers(layers)
    S = np.zeros_like(a)
    rec = None if records is None else np.ascontiguousarray(records)
    assert rec is None or rec.nbytes == 32 * W * H
    assert lib.rpt_glare_oracle_stage(a.ctypes.data, W, H, int(bool(wrap)), None if rec is None else rec.ctypes.data, len(layers), w.ctypes.data,
                                      taps.ctypes.data, radius.ctypes.data, S.ctypes.data) == 0
    return S


def wraps(camera):
    """The splat's `wrap`: a full-circle panorama."""
    return camera.get("mode", "pinhole") == "equirect" and np.float32(camera.get("h_fov", 2.0 * np.pi)) == np.float32(2.0 * np.pi)


def glared(lib, plain, W, H, layers, pixels, records, white_point, wrap, star_pass=False):
    """A pass with glare on, in C: `plain(scratch, records)` calls one of the library's plain pass functions through its cases module
    (it returns (frame, counts, ...)); its accumulator is kept (glare_oracle.c), rules G2-G5 run on it — masked by the records in the
    star pass — and rule G6 on a copy of `pixels`.  (the frame, (the plain pass's first count, pixels changed), S, the accumulator)"""
    words = W * H * 3
    assert lib.rpt_glare_oracle_arm(words) == 0
    plain_counts = plain(np.ascontiguousarray(pixels).copy(), records)[1]
    acc = np.zeros((H, W, 3), dtype=np.uint64)
    assert lib.rpt_glare_oracle_captured(acc.ctypes.data, words) == 0, "the plain pass did not allocate and free an accumulator of this frame's size"
    S = oracle_stage(lib, acc, layers, records if star_pass else None, wrap)
    out = np.ascontiguousarray(pixels).copy()
    assert out.nbytes == 16 * W * H
    wp = np.ascontiguousarray(white_point, dtype=np.float32)
    changed = C.c_uint64(0)
    assert lib.rpt_glare_oracle_resolve(S.ctypes.data, W, H, wp.ctypes.data, out.ctypes.data, C.byref(changed)) == 0
    return out, (plain_counts[0], int(changed.value)), S, acc


def random_accumulator(W, H, rng, lit=0.15):
    """(H, W, 3) uint64: most words zero, the rest spread over 1 .. 2^40 in magnitude, a few above the clamp of rule G2, and one stretch
    of a row and one block all lit (no wave of kernel 1170 would skip there)."""
    a = np.zeros((H, W, 3), dtype=np.uint64)
    on = rng.random((H, W)) < lit
    mag = np.exp2(rng.uniform(0.0, 40.0, size=(H, W, 3)))
    a[on] = mag[on].astype(np.uint64)
    a[H // 2, : W // 2] = (np.exp2(rng.uniform(20.0, 30.0, size=(W // 2, 3)))).astype(np.uint64)
    a[: H // 3, W // 3: W // 3 + 5] = np.uint64(1) << np.uint64(33)
    for _ in range(6):
        a[rng.integers(H), rng.integers(W), rng.integers(3)] = (np.uint64(1) << np.uint64(44)) + np.uint64(rng.integers(1, 1 << 40))
    a[0, 0] = np.uint64(1) << np.uint64(50)
    a[H - 1, W - 1] = np.uint64(12345678901)
    return a


def spread_colours(n, rng):
    """(n, 3) float32 colours spread over 1e-2 .. 1e6, log-uniform."""
    return np.exp(rng.uniform(np.log(1e-2), np.log(1e6), size=(n, 3))).astype(np.float32)
