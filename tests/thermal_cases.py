"""The thermal point sources' test infrastructure: the ctypes face of tests/native/thermal_oracle.c, the numpy float32
restatement of T_f that the device probe must equal bit for bit, the derived error bound, the probe's inputs, and the catalogues, sets
and temperatures of the parity cases — shared by tests/test_thermal_model.py (no GPU: the C operator against the float64 model, and the
non-vacuity of the cases here on CPU event frames) and tests/test_gpu_thermal_*.py (which run exactly these on the device)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
from relativitypathtracer_amd import particles, stars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "thermal_oracle.c")

F = np.float32
U = 2.0 ** -24                      # float32's unit roundoff
NU_R, NU_B = F(546.1 / 700.0), F(546.1 / 435.8)
T_MIN, T_MAX = 500.0, 1e8
FLAGS = [0, 1, 2, 3]
SEED = 23

SIZES = sc.SIZES                    # 128 x 72 and 67 x 41
CAMERAS = {k: sc.CAMERAS[k] for k in ("pinhole", "sphere")}     # the pinhole and the full-circle equirect
MOTIONS = ["rest", "0.9c"]
INTERVALS = [-1, 0]
SCENE = "cubes"


# ---- the C oracle ------------------------------------------------------------------------------------------------------------------
def _build(directory, define, name):
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/thermal_oracle.c")
    so = os.path.join(str(directory), name)
    p = subprocess.run(["gcc", *eo.CFLAGS, define, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_thermal_oracle_colour.restype = C.c_int
    lib.rpt_thermal_oracle_colour.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_thermal_oracle_x_green.restype = C.c_int
    lib.rpt_thermal_oracle_x_green.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def build_stars_library(directory) -> C.CDLL:
    lib = _build(directory, "-DTHERMAL_STARS", "libthermal_stars_oracle.so")
    # (stars_oracle.c's own entry points, as stars_cases binds them: sc.oracle_place and sc.oracle_pass take this library too)
    lib.rpt_stars_oracle_place.restype = C.c_int
    lib.rpt_stars_oracle_place.argtypes = [C.POINTER(sc.StarsView), C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_stars_oracle_pass.restype = C.c_int
    lib.rpt_stars_oracle_pass.argtypes = [C.POINTER(sc.StarsView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_thermal_oracle_stars_colours.restype = C.c_int
    lib.rpt_thermal_oracle_stars_colours.argtypes = [C.POINTER(sc.StarsView), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_thermal_oracle_stars_pass.restype = C.c_int
    lib.rpt_thermal_oracle_stars_pass.argtypes = [C.POINTER(sc.StarsView), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def build_particles_library(directory) -> C.CDLL:
    lib = _build(directory, "-DTHERMAL_PARTICLES", "libthermal_particles_oracle.so")
    # (particles_oracle.c's own entry points, as particles_cases binds them: pc.oracle_place and pc.oracle_pass take this library too)
    lib.rpt_particles_oracle_place.restype = C.c_int
    lib.rpt_particles_oracle_place.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_particles_oracle_pass.restype = C.c_int
    lib.rpt_particles_oracle_pass.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_thermal_oracle_particles_colours.restype = C.c_int
    lib.rpt_thermal_oracle_particles_colours.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_thermal_oracle_particles_pass.restype = C.c_int
    lib.rpt_thermal_oracle_particles_pass.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def probe_records(D, rgb, flags, xg) -> np.ndarray:
    """(n, 6) float32 {D, r, g, b, flags, x_G}: what rpt_probe which = 8 and rpt_thermal_oracle_colour take."""
    D = np.asarray(D, dtype=np.float32).reshape(-1)
    rec = np.zeros((len(D), 6), dtype=np.float32)
    rec[:, 0], rec[:, 1:4], rec[:, 4], rec[:, 5] = D, np.asarray(rgb, dtype=np.float32).reshape(-1, 3), flags, np.asarray(xg, dtype=np.float32)
    return rec


def oracle_colour(lib, D, rgb, flags, xg) -> np.ndarray:
    rec = probe_records(D, rgb, flags, xg)
    out = np.zeros((len(rec), 3), dtype=np.float32)
    assert lib.rpt_thermal_oracle_colour(rec.ctypes.data, len(rec), out.ctypes.data) == 0
    return out


def oracle_x_green(lib, kelvin) -> np.ndarray:
    T = np.ascontiguousarray(kelvin, dtype=np.float32).reshape(-1)
    out = np.zeros(len(T), dtype=np.float32)
    assert lib.rpt_thermal_oracle_x_green(T.ctypes.data, len(T), out.ctypes.data) == 0
    return out


def x_green32(kelvin) -> np.ndarray:
    """What the library uploads for float32 temperatures: stars.x_green (float64) rounded to float once."""
    return stars.x_green(np.asarray(kelvin, dtype=np.float32)).astype(np.float32)


def oracle_stars_colours(lib, v, catalogue, xg):
    """Rules 1-3 per star with temperatures: dict of visible (by rules 1-3 and 4), rgb after rule 3, D."""
    cat = np.ascontiguousarray(catalogue, dtype=stars.STAR_DTYPE)
    x = np.ascontiguousarray(xg, dtype=np.float32)
    out = np.zeros((len(cat), 5), dtype=np.float32)
    assert len(x) == len(cat) and lib.rpt_thermal_oracle_stars_colours(C.byref(v), cat.ctypes.data, x.ctypes.data, len(cat), out.ctypes.data) == 0
    return {"visible": out[:, 0] != 0, "rgb": out[:, 1:4], "D": out[:, 4]}


def oracle_stars_pass(lib, v, catalogue, xg, pixels, records):
    """Rules 1-6 with temperatures: (the framebuffer after the pass — a copy —, (stars inside, pixels changed))."""
    cat = np.ascontiguousarray(catalogue, dtype=stars.STAR_DTYPE)
    x = np.ascontiguousarray(xg, dtype=np.float32)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert len(x) == len(cat) and out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    counts = (C.c_uint64 * 2)()
    assert lib.rpt_thermal_oracle_stars_pass(C.byref(v), cat.ctypes.data, x.ctypes.data, len(cat), out.ctypes.data, rec.ctypes.data, counts) == 0
    return out, (int(counts[0]), int(counts[1]))


def oracle_particles_colours(lib, v, objects, ps, xg, windows=None):
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    x = np.ascontiguousarray(xg, dtype=np.float32)
    keep, wp = pc._windows_ptr(windows)
    out = np.zeros((len(ps), 5), dtype=np.float32)
    assert len(x) == len(ps)
    assert lib.rpt_thermal_oracle_particles_colours(C.byref(v), obj.ctypes.data, obj.size // 320, wp, ps.ctypes.data, x.ctypes.data, len(ps), out.ctypes.data) == 0
    del keep
    return {"visible": out[:, 0] != 0, "rgb": out[:, 1:4], "D": out[:, 4]}


def oracle_particles_pass(lib, v, objects, ps, xg, pixels, records, windows=None):
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    x = np.ascontiguousarray(xg, dtype=np.float32)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert len(x) == len(ps) and out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    keep, wp = pc._windows_ptr(windows)
    counts = (C.c_uint64 * 2)()
    assert lib.rpt_thermal_oracle_particles_pass(C.byref(v), obj.ctypes.data, obj.size // 320, wp, ps.ctypes.data, x.ctypes.data, len(ps), out.ctypes.data,
                                                 rec.ctypes.data, counts) == 0
    del keep
    return out, (int(counts[0]), int(counts[1]))


# ---- T_f in numpy float32, operation for operation ------------------------------------------------------------------
def exp32(z):
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        zero = ~(z > F(-86.0))
        zc = np.where(zero, F(0.0), np.where(z > F(88.0), F(88.0), z)).astype(np.float32)
        t = zc * F(1.4426950408889634)
        k = (t + np.where(t < F(0.0), F(-0.5), F(0.5)).astype(np.float32)).astype(np.int32)        # (truncates, as C's (int) does)
        kf = k.astype(np.float32)
        r = (zc - kf * F(0.693359375)) - kf * F(-2.12194440e-4)
        p = np.full_like(r, F(1.0 / 5040.0))
        for c in (F(1.0 / 720.0), F(1.0 / 120.0), F(1.0 / 24.0), F(1.0 / 6.0), F(0.5), F(1.0), F(1.0)):
            p = p * r + c
        scale = ((k + np.int32(127)) << np.int32(23)).astype(np.int32).view(np.float32)
        out = p * scale
    return np.where(zero, F(0.0), out).astype(np.float32)


def one_minus_exp32(z):
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(all="ignore"):
        big = z > F(0.5)
        from_exp = F(1.0) - exp32(-z)
        p = np.full_like(z, F(1.0 / 362880.0))
        for c in (F(1.0 / 40320.0), F(1.0 / 5040.0), F(1.0 / 720.0), F(1.0 / 120.0), F(1.0 / 24.0), F(1.0 / 6.0), F(0.5), F(1.0)):
            p = c - z * p
        series = z * p
    return np.where(big, from_exp, series).astype(np.float32)


def ratio32(x, D):
    with np.errstate(all="ignore"):
        y = (x / D).astype(np.float32)
        return ((exp32(x - y) * one_minus_exp32(x)) / one_minus_exp32(y)).astype(np.float32)


def T32(D, rgb, flags, xg):
    """T_f(flags, D, c, x_G) in float32; D (n,), rgb (n, 3), flags scalar or (n,), xg (n,).  Returns (n, 3) float32."""
    from doppler_model import S32
    D = np.asarray(D, dtype=np.float32).reshape(-1)
    rgb = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    xg = np.asarray(xg, dtype=np.float32).reshape(-1)
    flags = np.broadcast_to(np.asarray(flags, dtype=np.int64), D.shape)
    plain = S32(D, rgb, flags)
    with np.errstate(all="ignore"):
        q = np.stack([ratio32(xg * NU_R, D), ratio32(xg, D), ratio32(xg * NU_B, D)], axis=1)
        d3 = ((D * D) * D)[:, None]
        q = np.where(((flags & 2) == 0)[:, None], q / d3, q).astype(np.float32)
        thermal = (rgb * q).astype(np.float32)
    thermal = np.where((D == F(1.0))[:, None], rgb, thermal)
    return np.where(((xg == F(0.0)) | ((flags & 1) == 0))[:, None], plain, thermal).astype(np.float32)


# ---- the derived bound ("Error") --------------------------------------------------------------------------------------
def relative_bound(x, D):
    """The relative error of one channel of T_f in float32 against the real-number value, as DESIGN.md §21 derives it operation by
    operation, for x = x_k (float64) and D: (3 x + 4 y + |x - y| + 30) u, y = x / D, u = 2^-24.  The first three terms are the absolute
    error of the exponent x - y (x_k carries 3 roundings, y 4, the difference one more); the constant collects the exponential (3), the
    two 1 - e^-z (6 each, with 3 and 4 more from their arguments' errors), the product and the quotient (2), D^3 and its division (3),
    the colour's product (1) — 28 — and 2 for the terms of second order."""
    x = np.asarray(x, dtype=np.float64)
    y = x / np.asarray(D, dtype=np.float64)
    return (3.0 * x + 4.0 * y + np.abs(x - y) + 30.0) * U


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def operator_inputs(n_random, rng):
    """(D, rgb, T) for the operator's tests: D exactly 1 and next to it, D log-uniform over [1e-3, 1e3] and at both ends; T log-uniform
    over [500, 1e8] and at both ends; colours zero, in [0, 1] and above 1."""
    one = F(1.0)
    Ds = [one, np.nextafter(one, F(0)), np.nextafter(one, F(2)), F(1e-3), F(1e3), F(0.5), F(2.0), F(9.9), F(0.1)]
    Ts = [F(T_MIN), F(T_MAX), np.nextafter(F(T_MIN), F(np.inf)), np.nextafter(F(T_MAX), F(0)), F(3000.0), F(5772.0), F(12000.0)]
    grid_D, grid_T = np.meshgrid(np.repeat(np.array(Ds, dtype=np.float32), 8), np.array(Ts, dtype=np.float32), indexing="ij")       # (8 colours each)
    D = np.concatenate([grid_D.reshape(-1), np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n_random)).astype(np.float32)])
    T = np.concatenate([grid_T.reshape(-1), np.exp(rng.uniform(np.log(T_MIN), np.log(T_MAX), n_random)).astype(np.float32)])
    T = np.clip(T, F(T_MIN), F(T_MAX))
    ends = rng.random(len(T)) < 0.05
    T[ends] = np.where(rng.random(int(ends.sum())) < 0.5, F(T_MIN), F(T_MAX))
    n = len(D)
    c = rng.uniform(0, 1, size=(n, 3)).astype(np.float32)
    c[rng.random(n) < 0.2] *= F(40.0)
    c[rng.random(n) < 0.05] = 0.0
    c[rng.random((n, 3)) < 0.05] = 0.0
    return D, c, T


def probe_inputs(n, rng):
    """(D, rgb, x_G), n of each, for the device probe: operator_inputs' grid through the host's conversion, plus x_G = 0 (S_f), x_G next
    to 0 (1e-30, 1e-6), at the range's ends (T = 1e8 and T = 500) and one float inside and outside each."""
    D, c, T = operator_inputs(n, rng)
    xg = x_green32(T)
    lo, hi = x_green32([T_MAX])[0], x_green32([T_MIN])[0]
    special = np.array([0.0, 1e-30, 1e-6, lo, np.nextafter(lo, F(0)), np.nextafter(lo, F(1)), hi, np.nextafter(hi, F(0)), np.nextafter(hi, F(100))],
                       dtype=np.float32)
    pick = rng.random(len(xg)) < 0.1
    xg[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    keep = rng.permutation(len(D))[:n]
    return D[keep], c[keep], xg[keep]


def temperatures(n, rng, cold_every=3):
    """n temperatures for a parity case: log-uniform over 3000 .. 12000 K, every cold_every-th 0 (the source keeps S_f), the first few at
    the range's ends."""
    T = np.exp(rng.uniform(np.log(3000.0), np.log(12000.0), n)).astype(np.float32)
    T[::cold_every] = 0.0
    T[1:8:3] = T_MIN
    T[2:9:3] = T_MAX
    return T


def miss_pixel(records, W, H):
    """A miss pixel of a view's records, away from the frame's edge: where the 1000 stars on one pixel go."""
    hit = (np.ascontiguousarray(records).reshape(-1)["object"] >= 0).reshape(H, W)
    assert hit.any() and (~hit).any()
    miss = np.nonzero(~hit[2:H - 2, 2:W - 2])
    return int(miss[1][0]) + 2, int(miss[0][0]) + 2


def star_case(camera, W, H, E, interval, pile=None):
    """(catalogue, temperatures, {what: slice}): stars_cases' 2000 random stars and crafted ones, with a temperature each — the random
    ones as temperatures() has them; the crafted groups thermal except every other star on the frame's edges; the pile of 1000 on one
    pixel at 4500 K; the zero colour, the 1e30 and the out-of-band red star (which S_f blacks out at 0.9c) thermal."""
    cat, groups = sc.catalogue(camera, W, H, E, interval, pile)
    T = temperatures(len(cat), np.random.default_rng(SEED))
    for what, s in groups.items():
        T[s] = 6000.0
    e = groups["edges and corners"]
    T[e.start:e.stop:2] = 0.0
    T[groups["pile"]] = 4500.0
    T[groups["out of band"]] = 3500.0
    cat["rgb"][groups["out of band"]] = stars.blackbody_rgb(3500.0)         # (T_f scales each channel: it needs all three to show)
    return cat, T, groups


def particle_case(records, objects, camera, W, H, interval):
    """(set, temperatures, {what: slice}, bias): 2000 random particles in front of what the frame sees plus particles_cases' crafted
    ones built from the view's own records, with a temperature each, as star_case gives them."""
    rng = np.random.default_rng(SEED + 1)
    crafted, groups, bias = pc.crafted(records, objects, camera, W, H, interval)
    rec = np.ascontiguousarray(records).reshape(-1)
    hit = rec["object"] >= 0
    o = int(rec["object"][hit][0])
    x, y = rng.uniform(-0.5, W - 0.5, 2000), rng.uniform(-0.5, H - 0.5, 2000)
    d = rng.uniform(0.3, 0.9, 2000) * float(rec["dist"][hit].min())
    n = sc.pixel_direction(camera, W, H, x, y)
    base = particles.from_arrays(pc.rest_position(objects, o, n, d, interval), o, stars.blackbody_rgb(rng.uniform(3000.0, 12000.0, 2000)) * 0.2)
    ps = np.concatenate([base, crafted])
    groups = {k: slice(s.start + len(base), s.stop + len(base)) for k, s in groups.items()}
    T = temperatures(len(ps), rng)
    for what, s in groups.items():
        T[s] = 6000.0
    e = groups["edges and corners"]
    T[e.start:e.stop:2] = 0.0
    T[groups["pile"]] = 4500.0
    s = groups["surface"]
    T[s.start:s.stop:2] = 0.0
    return ps, T, groups, bias
