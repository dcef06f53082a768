"""The scenes, clouds and windows of the lit-particle tests, and the ctypes face of tests/native/dust_oracle.c — TEST INFRASTRUCTURE shared
by tests/test_dust_model.py (no GPU: the C oracle against the float64 model, and the non-vacuity of the cases here) and
tests/test_gpu_dust.py (which runs exactly these on the device's own frames)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
import oracle_ffi
import particles_cases as pc
from relativitypathtracer_amd import particles
from relativitypathtracer_amd.events import _objects_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "dust_oracle.c")
LIT, SHADOWED, AMBIENT = particles.LIT, particles.SHADOWED, particles.AMBIENT
LIGHTINGS = [LIT, LIT | SHADOWED, LIT | AMBIENT, LIT | SHADOWED | AMBIENT]
CLEARANCE = 1e-2                             # every grain of a cloud is at least this far from any surface at rest
# shadows.txt: 0 the lamp (a sphere of radius 0.5 at 0.95c along +x), 1 the floor, 2 the red sphere, 3 the back wall, 4 the pear
LAMP, FLOOR, SPHERE, WALL, PEAR = 0, 1, 2, 3, 4
SPHERE_CENTRE, PEAR_CENTRE = np.array([-4.0, -2.5, 8.0]), np.array([2.0, -1.5, 12.0])
BOX = (np.array([-7.0, -3.4, 4.0]), np.array([7.0, 4.0, 14.0]))      # the cloud's box in the frame of the objects at rest
LIGHT_TEXT = ("Os\n p-2,3,6,0,0,0,0,0.3,0.3,0.3\n l1\n c8,8,8\n v0.5,0,0\n",
              "Os\n p3,-2,9,0,0,0,0,0.2,0.2,0.2\n l1\n c2,6,9\n",
              "Os\n p-1,1,12,0,0,0,0,0.25,0.25,0.25\n l1\n c9,3,2\n v0,0,-0.8\n")


def build_library(directory) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/dust_oracle.c")
    so = os.path.join(str(directory), "libdust_oracle.so")
    p = subprocess.run(["gcc", *eo.CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_dust_oracle_pass.restype = C.c_int
    lib.rpt_dust_oracle_pass.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.POINTER(pc.ParticlesView), C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_dust_oracle_pairs.restype = C.c_int
    lib.rpt_dust_oracle_pairs.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    # the plain pass of the same library (particles_oracle.c is part of it): what "off means off" and interval 0 are held to
    lib.rpt_particles_oracle_pass.restype = C.c_int
    lib.rpt_particles_oracle_pass.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_particles_oracle_place.restype = C.c_int
    lib.rpt_particles_oracle_place.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    return lib


_SCENES = {}


def scene(name, motion="rest", interval=-1, lights=1):
    """`shadows` as shipped, or `cubes` with `lights` (0 .. 3) lamps of LIGHT_TEXT added behind its 34 cubes."""
    key = (name, motion, interval, lights)
    if key not in _SCENES:
        if name == "shadows":
            _SCENES[key] = eo.load_scene("shadows", motion, interval)
        else:
            with open(os.path.join(ROOT, "assets", "reference", "Scenes", "cubes.txt")) as f:
                text = f.read()
            head, tail = text.split("TTextures", 1)
            text = head + "".join(LIGHT_TEXT[:lights]) + "TTextures" + tail
            _SCENES[key] = eo.scene_from_text(text, eo.CAMERAS[motion], eo.SCENE_TIMES["cubes"] if motion == "rest" else 0.0, interval)
    return _SCENES[key]


def pear_radius(s):
    """The largest |coordinate| of the pear's vertices about its centre (its scale is 1): a cube of that half-edge holds it."""
    v = s.buffers()["vertices"][:, :3].astype(np.float64)
    return float(np.abs(v).max())


def clearance(objects, ps):
    """How far every grain is from the surface of every sphere and cube of Object[], at the grain's own event — the event the frame sees
    it at, which is also where its shadow rays start — in float64: (N, n_obj), NaN for a mesh.  Per object i the event goes into i's rest
    frame (Lorentz_i of the grain's event in the camera frame, particles.illuminate's hit_pos) and into its unit space (InvM_i); there
    the distance to the unit sphere or the unit cube is taken (inside a cube: to its nearest face) and scaled by the SMALLEST of the
    object's three scales, so the figure is a lower bound of the rest-frame distance."""
    objs = _objects_array(objects)
    hit = particles.illuminate(ps, objs, -1, 0, 0.0, LIT)["hit_pos"]
    out = np.full((len(hit), len(objs)), np.nan)
    for i in range(len(objs)):
        if objs["type"][i] not in (0, 1):
            continue
        P = hit @ objs["Lorentz"][i].astype(np.float64).reshape(4, 4).T
        inv_m = objs["InvM"][i].astype(np.float64).reshape(4, 4)
        q = P[:, 1:] @ inv_m[:3, :3].T + inv_m[:3, 3]
        scale = float(np.linalg.norm(objs["M"][i].astype(np.float64).reshape(4, 4)[:3, :3], axis=0).min())
        if objs["type"][i] == 0:
            d = np.abs(np.linalg.norm(q, axis=1) - 1.0)
        else:
            a = np.abs(q)
            outside = np.linalg.norm(np.maximum(a - 1.0, 0.0), axis=1)
            d = np.where(a.max(axis=1) > 1.0, outside, 1.0 - a.max(axis=1))
        out[:, i] = d * scale
    return out


def cloud(name, s, count, seed=3, albedo=(0.8, 0.7, 0.6)):
    """`count` grains at most: particles.dust in BOX riding an object at rest (shadows: the floor; cubes: cube 0), every grain at least
    CLEARANCE from every surface: more than 2 CLEARANCE from every sphere and cube at the grain's own event (`clearance`), and for shadows
    outside the cube that holds the pear; for shadows also grains riding the lamp and the red sphere around them."""
    host = FLOOR if name == "shadows" else 0
    ps = particles.dust(host, BOX[0], BOX[1], count, albedo, seed)
    pos = ps["pos"].astype(np.float64)
    if name == "shadows":
        def clear(q):
            q = q["pos"].astype(np.float64)
            return (np.linalg.norm(q - SPHERE_CENTRE, axis=1) > 1.0 + 2 * CLEARANCE) & (np.abs(q - PEAR_CENTRE).max(axis=1) > pear_radius(s) + 2 * CLEARANCE)
        ps = ps[clear(ps)]
        n_ride = max(1, len(ps) // 16)
        ride = particles.dust(LAMP, np.array([-5.0, -3.0, 10.0]) - 2.0, np.array([-5.0, -3.0, 10.0]) + 2.0, n_ride, (0.5, 0.9, 0.7), seed + 1)
        ride = ride[np.linalg.norm(ride["pos"].astype(np.float64) - np.array([-5.0, -3.0, 10.0]), axis=1) > 0.5 + 2 * CLEARANCE]
        # ... and grains riding the red sphere around it: those behind it, seen from the lamp, are shadowed by their own host alone
        own = particles.dust(SPHERE, SPHERE_CENTRE - 2.5, SPHERE_CENTRE + 2.5, n_ride, (0.9, 0.5, 0.5), seed + 2)
        own = own[clear(own) & (own["pos"][:, 1] > -3.4)]
        ps = np.concatenate([ps[:len(ps) - len(ride) - len(own)], ride, own])
    # every sphere and cube, moving or not, where it is at the grain's own event — a grain riding the lamp may pass the floor's face, a
    # grain at rest a moving cube's — (the cloud therefore depends on the camera's motion)
    ps = ps[np.nanmin(clearance(s, ps), axis=1) > 2 * CLEARANCE]
    return np.ascontiguousarray(ps)


def _windows_ptr(windows):
    if windows is None:
        return None, None
    w = np.ascontiguousarray(windows, dtype=np.float32).reshape(-1)
    return w, w.ctypes.data


def oracle_pass(lib, s, v, objects, lighting, ps, pixels, records, windows=None):
    """Rules D0-D7 and §20's 5-6: (the framebuffer after the pass — a copy —, (seen, changed), (pairs lit, pairs shadowed))."""
    a, keep = eo.oracle_args(s, v.width, v.height, objects, v.interval)
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    wkeep, wp = _windows_ptr(windows)
    counts = (C.c_uint64 * 4)()
    assert lib.rpt_dust_oracle_pass(C.byref(a), C.byref(v), lighting, wp, ps.ctypes.data, len(ps), out.ctypes.data, rec.ctypes.data, counts) == 0
    del keep, wkeep
    return out, (int(counts[0]), int(counts[1])), (int(counts[2]), int(counts[3]))


def oracle_pairs(lib, s, objects, doppler, lighting, ps, windows=None):
    """D1-D6 for every grain, seen or not, and every object: state (N, n_obj) — 0 no light, 1 lit, 2 skipped for len, 3 outside the
    light's window, 4 shadowed, -1 no event —, te, len, k, di, contribution (N, n_obj, 3), mask (N, n_obj) uint64 of ALL occluders,
    c_rest (N, 3)."""
    a, keep = eo.oracle_args(s, 1, 1, objects, -1)
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    n, no = len(ps), a.object_count
    pairs = np.zeros((n, no, 8), dtype=np.float32)
    masks = np.zeros((n, no), dtype=np.uint64)
    c_rest = np.zeros((n, 3), dtype=np.float32)
    wkeep, wp = _windows_ptr(windows)
    assert lib.rpt_dust_oracle_pairs(C.byref(a), doppler, lighting, wp, ps.ctypes.data, n, pairs.ctypes.data, masks.ctypes.data, c_rest.ctypes.data) == 0
    del keep, wkeep
    return {"state": pairs[:, :, 0].astype(np.int64), "te": pairs[:, :, 1], "len": pairs[:, :, 2], "k": pairs[:, :, 3], "di": pairs[:, :, 4],
            "contribution": pairs[:, :, 5:8], "mask": masks, "c_rest": c_rest}


def shadows_windows(lib, s, objects, ps):
    """The windowed case on `shadows`: the lamp switched on at t0 (its rest frame) and the red sphere ending at t1 (its own), chosen from the
    oracle's own numbers so that the lamp is windowed out for some grains and not for others, and the sphere's shadow is there for some
    grains and gone for others.  (n_obj, 2) float32."""
    free = oracle_pairs(lib, s, objects, 0, LIT | SHADOWED, ps)
    te = free["te"][:, LAMP][free["state"][:, LAMP] > 0]
    t0 = float(np.median(te))
    windows = np.tile(np.array([-np.inf, np.inf], dtype=np.float32), (len(objects), 1))
    windows[LAMP, 0] = t0
    by_sphere = int(((free["mask"][:, LAMP] >> np.uint64(SPHERE)) & np.uint64(1)).sum())
    T = float(_objects_array(objects)["stationaryCam"][SPHERE].reshape(4)[0])
    full = int(((oracle_pairs(lib, s, objects, 0, LIT | SHADOWED, ps, windows)["mask"][:, LAMP] >> np.uint64(SPHERE)) & np.uint64(1)).sum())
    for t1 in np.linspace(T - 40.0, T, 81):
        windows[SPHERE, 1] = t1
        held = oracle_pairs(lib, s, objects, 0, LIT | SHADOWED, ps, windows)
        left = int(((held["mask"][:, LAMP] >> np.uint64(SPHERE)) & np.uint64(1)).sum())
        if 0 < left < full:
            return windows
    raise AssertionError(f"no end time of the red sphere leaves part of its shadow ({by_sphere} grains in it without windows)")
