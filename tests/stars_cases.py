"""The scenes, cameras, sizes and catalogues of the star-field tests, and the ctypes face of tests/native/stars_oracle.c — TEST
INFRASTRUCTURE shared by tests/test_stars_model.py (no GPU: the C oracle against the float64 model, and the non-vacuity of the cases
here on CPU event frames) and tests/test_gpu_stars.py (which runs exactly these on the device)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
from relativitypathtracer_amd import stars
from relativitypathtracer_amd.renderer import orient_matrix, orient_objects, rotation_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "stars_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's

SIZES = [(128, 72), (67, 41)]                # 67 x 41: odd, no multiple of a 256-lane workgroup's pixels per row
YPR = (0.2, -0.1, 0.15)
LENS_V_FOV = 1.2
CAMERAS = {"pinhole": dict(mode="pinhole"),
           "lens": dict(mode="pinhole", v_fov=LENS_V_FOV, orientation=YPR),      # the lens turned by YPR
           "sphere": dict(mode="equirect"),                                      # the full sphere: column taps wrap
           "partial": dict(mode="equirect", h_fov=3.0, v_fov=1.2, yaw=0.1)}
SCENES = ["cubes", "arch"]
MOTIONS = ["rest", "0.9c"]                   # events_oracle.CAMERAS
FLAGS = [0, 1, 2, 3]                         # RPT_DOPPLER_SHIFT | RPT_DOPPLER_BEAMING
INTERVALS = [-1, 0]
SEED = 11


class StarsView(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("interval", C.c_int), ("doppler", C.c_int), ("camera", C.c_int),
                ("lens_scale", C.c_float), ("h_fov", C.c_float), ("v_fov", C.c_float), ("yaw", C.c_float),
                ("white_point", C.c_float * 3), ("E", C.c_float * 16)]


def build_library(directory) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/stars_oracle.c")
    so = os.path.join(str(directory), "libstars_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_stars_oracle_matrix.restype = C.c_int
    lib.rpt_stars_oracle_matrix.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_stars_oracle_place.restype = C.c_int
    lib.rpt_stars_oracle_place.argtypes = [C.POINTER(StarsView), C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_stars_oracle_pass.restype = C.c_int
    lib.rpt_stars_oracle_pass.argtypes = [C.POINTER(StarsView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_stars_oracle_sky_direction.restype = C.c_int
    lib.rpt_stars_oracle_sky_direction.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return lib


def view(camera, W, H, E, interval, flags, white_point=(1.0, 1.0, 1.0)) -> StarsView:
    """The oracle's view of one of CAMERAS (or any mapping stars.project takes): E is the sky matrix as set on the context; the
    orientation re-bases it here through rpt_orient_matrix, as a launch does."""
    v = StarsView()
    v.width, v.height, v.interval, v.doppler = W, H, interval, flags
    v.camera = 1 if camera.get("mode", "pinhole") == "equirect" else 0
    v.lens_scale = float(eo.lens_scale(camera["v_fov"])) if v.camera == 0 and camera.get("v_fov") else 1.0
    v.h_fov, v.v_fov, v.yaw = camera.get("h_fov", 2.0 * math.pi), camera.get("v_fov", math.pi), camera.get("yaw", 0.0)
    v.white_point[:] = white_point
    e = np.ascontiguousarray(E, dtype=np.float32).reshape(4, 4)
    if camera.get("orientation") is not None:
        e = orient_matrix(e, *camera["orientation"])
    v.E[:] = e.reshape(16).tolist()
    return v


def oracle_place(lib, v, catalogue):
    """Rules 1-4 per star: dict of visible, X, Y, rgb, D, n (float32 as the oracle computed them)."""
    cat = np.ascontiguousarray(catalogue, dtype=stars.STAR_DTYPE)
    out = np.zeros((len(cat), 10), dtype=np.float32)
    assert lib.rpt_stars_oracle_place(C.byref(v), cat.ctypes.data, len(cat), out.ctypes.data) == 0
    return {"visible": out[:, 0] != 0, "X": out[:, 1], "Y": out[:, 2], "rgb": out[:, 3:6], "D": out[:, 6], "n": out[:, 7:10]}


def oracle_pass(lib, v, catalogue, pixels, records):
    """Rules 1-6: (the framebuffer after the pass — a copy, all 16 bytes of every pixel —, (stars inside, pixels changed))."""
    cat = np.ascontiguousarray(catalogue, dtype=stars.STAR_DTYPE)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    counts = (C.c_uint64 * 2)()
    assert lib.rpt_stars_oracle_pass(C.byref(v), cat.ctypes.data, len(cat), out.ctypes.data, rec.ctypes.data, counts) == 0
    return out, (int(counts[0]), int(counts[1]))


def pixel_direction(camera, W, H, x, y):
    """The kernels' own pixel-to-direction map in float64, before the orientation: the direction pixel (x, y) looks along (x and y may
    be fractional: the pinhole's pixel x sits AT x, the panorama's centre at x + 0.5, so pass x - 0.5 there for a pixel's edge)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if camera.get("mode", "pinhole") == "equirect":
        h_fov, v_fov, yaw = (float(np.float32(camera.get(k, d))) for k, d in (("h_fov", 2.0 * math.pi), ("v_fov", math.pi), ("yaw", 0.0)))
        lon = yaw + h_fov * ((x + 0.5) / W - 0.5)
        lat = v_fov * ((y + 0.5) / H - 0.5)
        p = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
    else:
        s = float(eo.lens_scale(camera["v_fov"])) if camera.get("v_fov") else 1.0
        p = np.stack([s * (x / W - 0.5) * (W / H), s * (y / H - 0.5), np.full_like(x, 0.5)], -1)
    return p / np.linalg.norm(p, axis=-1, keepdims=True)


def sky_direction(camera, E, interval, n):
    """Where the sky lookup looks for camera direction n (float64): the spatial part of E diag(1, R) (interval, n), normalised."""
    e = np.array(E, dtype=np.float64).reshape(4, 4)
    if camera.get("orientation") is not None:
        turn = np.eye(4)
        turn[1:, 1:] = rotation_matrix(*camera["orientation"])
        e = e @ turn
    n = np.asarray(n, dtype=np.float64).reshape(-1, 3)
    k = np.concatenate([np.full((len(n), 1), float(interval)), n], axis=1) @ e.T
    return k[:, 1:] / np.linalg.norm(k[:, 1:], axis=1, keepdims=True)


def crafted(camera, W, H, E, interval, pile=None):
    """The crafted stars of the parity test for one view, as (catalogue, {what: slice}): on exact pixel positions, on each frame edge
    and corner, behind the pinhole, on the panorama's seam and at both poles, 1000 copies of one star on the pixel `pile` (default the
    frame's centre), a zero colour, a colour of 1e30, and a red star that a blue shift or a red shift moves out of the visible band."""
    groups, dirs, cols = {}, [], []

    def add(what, n, rgb):
        n = np.asarray(n, dtype=np.float64).reshape(-1, 3)
        groups[what] = slice(len(dirs), len(dirs) + len(n))
        dirs.extend(sky_direction(camera, E, interval, n).tolist())
        cols.extend(np.broadcast_to(np.asarray(rgb, dtype=np.float64), (len(n), 3)).tolist())

    panorama = camera.get("mode", "pinhole") == "equirect"
    half = 0.5 if panorama else 0.0             # a pixel's edge lies half a pixel before its centre
    px = np.array([(3, 2), (W // 2, H // 2), (W - 4, H - 3), (W // 3, 2 * H // 3), (1, H - 2)], dtype=np.float64)
    add("on pixels", pixel_direction(camera, W, H, px[:, 0], px[:, 1]), (0.8, 0.6, 0.4))
    xs = np.array([0, W - 1, 0, W - 1, W // 2, W // 2, 0, W - 1, -0.5, W - 0.5, W // 2, W // 2, -1.0, W], dtype=np.float64)
    ys = np.array([0, 0, H - 1, H - 1, 0, H - 1, H // 2, H // 2, H // 2, H // 2, -0.5, H - 0.5, H // 2, -1.0], dtype=np.float64)
    add("edges and corners", pixel_direction(camera, W, H, xs, ys), (0.5, 0.9, 0.7))
    add("behind", [(0.1, 0.1, -1.0), (0.0, 0.0, -1.0), (1.0, 0.0, -0.2), (0.0, 1.0, -0.05)], (1.0, 1.0, 1.0))
    yaw = float(camera.get("yaw", 0.0)) if panorama else 0.0
    seam = [(math.sin(yaw + math.pi), 0.0, math.cos(yaw + math.pi)), (math.sin(yaw + math.pi - 1e-7), 0.1, math.cos(yaw + math.pi - 1e-7)),
            (math.sin(yaw - math.pi + 1e-3), -0.2, math.cos(yaw - math.pi + 1e-3))]
    add("seam", seam, (0.9, 0.9, 0.2))
    add("poles", [(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (1e-4, 1.0, 1e-4), (-1e-5, -1.0, 1e-5)], (0.3, 0.6, 0.9))
    pile = (W // 2 + 5, H // 2 + 3) if pile is None else pile
    add("pile", np.repeat(pixel_direction(camera, W, H, pile[0] + 0.25, pile[1] + 0.25)[None, :], 1000, axis=0), (90.0, 70.0, 0.004))
    add("zero colour", pixel_direction(camera, W, H, 7.0, 5.0), (0.0, 0.0, 0.0))
    add("1e30", pixel_direction(camera, W, H, 9.3, 6.6), (1e30, 1e30, 1e30))
    add("out of band", pixel_direction(camera, W, H, W // 2 - half, H // 2 - half), (1.0, 0.0, 0.0))
    cat = np.zeros(len(dirs), dtype=stars.STAR_DTYPE)
    cat["dir"], cat["rgb"] = np.asarray(dirs), np.asarray(cols)
    return cat, groups


def catalogue(camera, W, H, E, interval, pile=None):
    """random_catalogue(2000, SEED) plus the crafted stars."""
    extra, groups = crafted(camera, W, H, E, interval, pile)
    base = stars.random_catalogue(2000, SEED)
    return np.concatenate([base, extra]), {k: slice(s.start + len(base), s.stop + len(base)) for k, s in groups.items()}


def setup_camera(r, camera):
    """One of CAMERAS on a Renderer."""
    r.set_orientation(*(camera.get("orientation") or (0.0, 0.0, 0.0)))
    if camera.get("mode", "pinhole") == "equirect":
        r.set_field_of_view(0.0)
        r.set_projection("equirect", **{k: camera[k] for k in ("h_fov", "v_fov", "yaw") if k in camera})
    else:
        r.set_field_of_view(camera.get("v_fov", 0.0))
        r.set_projection("pinhole")


def cpu_events(lib, scene, W, H, camera):
    """The (H, W) records of tests/native/event_oracle.c for one of CAMERAS."""
    objects = orient_objects(scene, *camera["orientation"]) if camera.get("orientation") is not None else None
    if camera.get("mode", "pinhole") == "equirect":
        kw = {k: camera[k] for k in ("h_fov", "v_fov", "yaw") if k in camera}
        return eo.oracle_events(lib, scene, W, H, dirs=eo.pano_dirs(W, H, **kw), objects=objects)
    s = eo.lens_scale(camera["v_fov"]) if camera.get("v_fov") else None
    return eo.oracle_events(lib, scene, W, H, dirs=eo.pinhole_dirs(W, H, s), objects=objects)
