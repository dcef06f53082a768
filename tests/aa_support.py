"""Shared by the adaptive anti-aliasing tests: the sample directions of every camera in the kernels' float32 steps, the CPU reference
with the sample loop (tests/native/aa_oracle.c) and the cases of the plain-pinhole comparison."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

import oracle_ffi
from relativitypathtracer_amd.renderer import projection_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "aa_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)

# The plain-pinhole comparison: every shipped scene at 128 x 72 (each has silhouettes there: tests/test_adaptive_model.py checks on
# the CPU that every 0 <= T < 255 case refines some pixels and leaves some), n in {2, 3}, T in {-1, 0, 8, 255}.
PLAIN_SIZE = (128, 72)
PLAIN_NS = (2, 3)
PLAIN_THRESHOLDS = (-1, 0, 8, 255)


def build_oracle(tmpdir):
    assert shutil.which("gcc") is not None, "gcc is needed to build tests/native/aa_oracle.c"
    so = os.path.join(str(tmpdir), "libaa_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_aa_oracle_render.restype = C.c_int
    lib.rpt_aa_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_int]
    return lib


def _sample_coords(W, H, n):
    """(H, W, n, n) float32 xs, ys: (float)x + (float)sx / (float)n and the same in y, sample index sy * n + sx."""
    y, x, sy, sx = np.meshgrid(np.arange(H), np.arange(W), np.arange(n), np.arange(n), indexing="ij")
    fn = np.float32(n)
    xs = x.astype(np.float32) + sx.astype(np.float32) / fn
    ys = y.astype(np.float32) + sy.astype(np.float32) / fn
    return xs.astype(np.float32), ys.astype(np.float32)


def lens_sample_dirs(W, H, n, v_fov=None):
    """(H W n n, 3) float32: lensCamRayDir's plane point at the fractional coordinates; v_fov None = the reference's lens (s = 1)."""
    xs, ys = _sample_coords(W, H, n)
    s = np.float32(1.0) if v_fov is None else np.float32(math.tan(0.5 * float(np.float32(v_fov))))
    fx2 = (xs / np.float32(W) - np.float32(0.5)) * (np.float32(W) / np.float32(H))
    fy2 = ys / np.float32(H) - np.float32(0.5)
    return np.ascontiguousarray(np.stack([s * fx2, s * fy2, np.full_like(fx2, 0.5)], -1).reshape(-1, 3).astype(np.float32))


def pano_sample_dirs(W, H, n, **kw):
    """(H W n n, 3) float32: sample (sx, sy) of pixel (x, y) is pixel (n x + sx, n y + sy) of the n W x n H panorama."""
    cols, rows = projection_tables(n * W, n * H, **kw)
    sl, cl = cols[None, :, 0], cols[None, :, 1]
    sp, cp = rows[:, None, 0], rows[:, None, 1]
    p = np.stack([cp * sl, np.broadcast_to(sp, (n * H, n * W)), cp * cl], -1).astype(np.float32)      # (nH, nW, 3)
    p = p.reshape(H, n, W, n, 3).transpose(0, 2, 1, 3, 4)                                             # (H, W, sy, sx, 3)
    return np.ascontiguousarray(p.reshape(-1, 3))


def oracle_supersampled(lib, scene, W, H, n, dirs, objects=None, env=None, flags=0):
    """The family's CPU reference with the sample loop: (pixels, rgb, hits) with hits[H W] = the pixel's samples that hit an object.
    env: (E 4 x 4, image) or None; flags: the Doppler flags, for the rays that hit (tests/native/doppler_oracle.c) and for the sky."""
    d, prm = scene.desc(), scene.params
    a = oracle_ffi.OracleArgs()
    if objects is not None:
        objects = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
        a.objects, a.object_count = objects.ctypes.data, objects.size // 320
    else:
        a.objects, a.object_count = d.objects, d.object_count
    a.vertices, a.normals, a.uvs = d.vertices, d.normals, d.uvs
    a.triangles, a.octrees, a.octreeTris = d.triangles, d.octrees, d.octreeTris
    a.textures, a.texture_bytes = d.textures, d.texture_bytes
    a.white_point = (C.c_float * 3)(*prm["white_point"])
    a.ambient, a.width, a.height, a.interval, a.msaa = prm["ambient"], W, H, prm["interval"], 1
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    hits = np.zeros(W * H, dtype=np.uint8)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    assert dirs.shape == (W * H * n * n, 3) and dirs.dtype == np.float32
    if env is None:
        rc = lib.rpt_aa_oracle_render(C.byref(a), dirs.ctypes.data, n, None, None, 0, 0, int(flags), hits.ctypes.data, THREADS)
    else:
        E, img = np.ascontiguousarray(env[0], dtype=np.float32), np.ascontiguousarray(env[1])
        rc = lib.rpt_aa_oracle_render(C.byref(a), dirs.ctypes.data, n, E.ctypes.data, img.ctypes.data, img.shape[1], img.shape[0], int(flags),
                                      hits.ctypes.data, THREADS)
    assert rc == 0
    return px, rgb, hits


def rgb8_of(px, W, H):
    return px["rgba"].reshape(H, W, 4)[:, :, :3]


def sky_image(W, H, seed=1):
    """A smooth gradient with a few one-texel markers over the upper two thirds of the sky, one flat colour below: sky pixels with
    colours of their own, and a region where even threshold 0 finds no edge."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(40 + 180 * x / max(W - 1, 1)), (30 + 200 * y / max(H - 1, 1)), (220 - 150 * ((x + y) % max(W, 2)) / max(W, 2))], -1).astype(np.uint8)
    img[(2 * H) // 3:] = (60, 90, 150)
    rng = np.random.default_rng(seed)
    for k in range(12):
        img[rng.integers(0, (2 * H) // 3), rng.integers(0, W)] = (255, 255 * (k & 1), 0)
    return np.ascontiguousarray(img)
