"""The ray-map camera's test cases — TEST INFRASTRUCTURE shared by tests/test_raymap_fill.py (no GPU) and tests/test_gpu_raymap.py: the
float64 restatement of rpt_raymap_fill (include/rpt.h), the three cameras the GPU tests render through, the scenes, and the CPU
references fed a map (tests/native/*.c take the camera ray per pixel, so none of them changes)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

import oracle_ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's, as tests/test_gpu_panorama.py
THREADS = min(16, os.cpu_count() or 1)
KINDS = {"fisheye": 0, "equisolid": 1, "stereographic": 2, "cube_strip": 3}
DEG = math.pi / 180.0

# the cube strip's face bases of include/rpt.h: forward, right, up per face, faces +x, -x, +y, -y, +z, -z
CUBE_FORWARD = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
CUBE_RIGHT = np.array([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], dtype=np.float64)
CUBE_UP = np.array([[0, 1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1], [0, 1, 0], [0, 1, 0]], dtype=np.float64)


def rho64(W, H, fit):
    """(X, Y, rho) of include/rpt.h in float64, each (H, W)."""
    S = float(min(W, H)) if fit == 0 else math.sqrt(float(W) * W + float(H) * H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    X = (2.0 * (x + 0.5) - W) / S
    Y = (2.0 * (y + 0.5) - H) / S
    return X, Y, np.sqrt(X * X + Y * Y)


def fill64(kind, W, H, fov=None, fit=0):
    """rpt_raymap_fill restated in float64 numpy: ((H, W, 3) float64 directions, (H, W) bool no-ray set).  fov is taken as the float the
    library is handed."""
    if kind == "cube_strip":
        y, x = np.mgrid[0:H, 0:W]
        f = x // H
        a = (2.0 * ((x - f * H) + 0.5) - H) / H
        b = (2.0 * (y + 0.5) - H) / H
        p = CUBE_FORWARD[f] + a[..., None] * CUBE_RIGHT[f] + b[..., None] * CUBE_UP[f]
        return p, np.zeros((H, W), dtype=bool)
    fov = float(np.float32(fov))
    X, Y, rho = rho64(W, H, fit)
    safe = np.where(rho > 0, rho, 1.0)
    if kind == "fisheye":
        theta = rho * fov / 2.0
    elif kind == "equisolid":
        theta = 2.0 * np.arcsin(np.minimum(rho * math.sin(fov / 4.0), 1.0))
    else:
        theta = 2.0 * np.arctan(rho * math.tan(fov / 4.0))
    st = np.sin(theta)
    p = np.stack([st * X / safe, st * Y / safe, np.cos(theta)], -1)
    p[rho == 0] = (0.0, 0.0, 1.0)
    none = rho > 1.0
    p[none] = 0.0
    return p, none


# ---- the three cameras of the GPU tests: (kind, W, H, fov, fit).  100 x 52 and 120 x 20 are no multiple of the 8 x 8 wave tile in either
# direction; 128 x 72 is one in both.
CAMERAS = {
    "fisheye180": ("fisheye", 100, 52, 180.0 * DEG, 0),
    "stereo300": ("stereographic", 128, 72, 300.0 * DEG, 1),
    "cube_strip": ("cube_strip", 120, 20, None, 0),
}


def camera_map(name):
    """(dirs (H, W, 3) float32 from the library's own rpt_raymap_fill, W, H)"""
    from relativitypathtracer_amd.renderer import raymap
    kind, W, H, fov, fit = CAMERAS[name]
    return (raymap(kind, W, H) if fov is None else raymap(kind, W, H, fov=fov, fit=fit)), W, H


def has_ray(dirs):
    return np.any(np.asarray(dirs).reshape(-1, 3) != 0, axis=1)


def oracle_dirs(dirs):
    """The map as the CPU references take it, (H W, 3) float32; a pixel without a ray gets +z so that the reference has something to
    normalise — what it computes there is not looked at."""
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float32).reshape(-1, 3)).copy()
    d[~has_ray(d)] = (0.0, 0.0, 1.0)
    return d


# ---- the scenes: shipped files, the camera at rest at the scene's own time or passing a chosen point at 0.9 c; chosen on the CPU
# references alone so that through every camera above at least 5 % of the ray pixels hit an object and at least 5 % miss
SCENES = {
    "cubes": dict(rest=dict(v=(0.0, 0.0, 0.0), t=3.0, p=(-1.0, -0.5, 2.5)), fast=dict(v=(0.0, 0.0, -0.9), t=0.0, p=(0.0, 0.0, 0.0))),
    "shadows": dict(rest=dict(v=(0.0, 0.0, 0.0), t=16.0, p=(0.0, 0.0, 0.0)), fast=dict(v=(0.9, 0.0, 0.0), t=0.0, p=(0.0, 0.0, 0.0))),
    "bunny": dict(rest=dict(v=(0.0, 0.0, 0.0), t=0.0, p=(-0.5, -1.5, 3.8)), fast=dict(v=(0.0, 0.0, -0.9), t=0.0, p=(0.0, 0.0, 0.0))),
}


def load_scene(name, motion):
    from relativitypathtracer_amd import Scene
    s = Scene.from_file(name)
    c = SCENES[name][motion]
    s.set_camera(c["v"], c["t"], c["p"])
    s.update_objects()
    return s


def build_native(directory, source):
    """tests/native/<source>.c as a shared library, with the flags the panorama test uses."""
    assert shutil.which("gcc") is not None, "gcc is needed to build tests/native/" + source + ".c"
    so = os.path.join(str(directory), "lib" + source + ".so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, os.path.join(ROOT, "tests", "native", source + ".c"), "-lm", "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return C.CDLL(so)


def oracle_args(scene, W, H, objects=None):
    d, prm = scene.desc(), scene.params
    a = oracle_ffi.OracleArgs()
    keep = None
    if objects is not None:
        keep = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
        a.objects, a.object_count = keep.ctypes.data, keep.size // 320
    else:
        a.objects, a.object_count = d.objects, d.object_count
    a.vertices, a.normals, a.uvs = d.vertices, d.normals, d.uvs
    a.triangles, a.octrees, a.octreeTris = d.triangles, d.octrees, d.octreeTris
    a.textures, a.texture_bytes = d.textures, d.texture_bytes
    a.white_point = (C.c_float * 3)(*prm["white_point"])
    a.ambient, a.width, a.height, a.interval, a.msaa = prm["ambient"], W, H, prm["interval"], 1
    return a, keep


def panorama_oracle(directory):
    lib = build_native(directory, "panorama_oracle")
    lib.rpt_panorama_oracle_render.restype = C.c_int
    lib.rpt_panorama_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def panorama_frame(lib, scene, W, H, dirs, objects=None):
    """(pixels[H W] 16 B, rgb[H, W, 3]) of rpt_panorama_oracle_render fed the map"""
    a, keep = oracle_args(scene, W, H, objects)
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    d = oracle_dirs(dirs)
    assert lib.rpt_panorama_oracle_render(C.byref(a), d.ctypes.data, 0, H, THREADS) == 0
    del keep
    return px, rgb


def environment_oracle(directory):
    lib = build_native(directory, "environment_oracle")
    lib.rpt_environment_oracle_render.restype = C.c_int
    lib.rpt_environment_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_int]
    return lib


def environment_frame(lib, scene, W, H, dirs, E, img, flags):
    a, keep = oracle_args(scene, W, H)
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    hit = np.zeros(W * H, dtype=np.uint8)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    E = np.ascontiguousarray(E, dtype=np.float32)
    img = np.ascontiguousarray(img)
    d = oracle_dirs(dirs)
    assert lib.rpt_environment_oracle_render(C.byref(a), d.ctypes.data, E.ctypes.data, img.ctypes.data, img.shape[1], img.shape[0],
                                             int(flags), hit.ctypes.data, THREADS) == 0
    del keep
    return px, rgb


def sentinel_pixels(W, H):
    """What a pixel without a ray is written as: {x, y, rgba = 0, 0, 0, 1}, the fourth dword 0 as in every pixel"""
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    y, x = np.mgrid[0:H, 0:W]
    px["x"], px["y"] = x.reshape(-1), y.reshape(-1)
    px["rgba"] = (0, 0, 0, 1)
    return px


def expected_frame(opx, orgb, dirs, W, H):
    """The reference's frame where the map has a ray, the sentinel pixel and a zero float triple where it has none"""
    ray = has_ray(dirs)
    px = np.where(ray, opx, sentinel_pixels(W, H))
    rgb = np.where(ray.reshape(H, W, 1), orgb, np.float32(0.0))
    return px, rgb
