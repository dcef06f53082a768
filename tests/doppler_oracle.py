"""Builds and binds tests/native/doppler_oracle.c — the CPU oracle with the Doppler and beaming of rpt_set_doppler restated for rays that
hit an object (DESIGN.md "Doppler and beaming") — and forms the camera rays of every camera in the kernels' float32 steps.  TEST
INFRASTRUCTURE: used by tests/test_doppler_oracle.py (no GPU), tests/test_gpu_doppler_parity.py and tests/golden/make_oracle_golden.py."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

import oracle_ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "doppler_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)

# the record of trace_doppler: the 11 floats of rpt_set_debug_doppler first, then what the float64 checks need
RECORD_DTYPE = np.dtype([("dcam", "<f4"), ("dlight", "<f4"), ("ref", "<f4", (3,)), ("lit", "<f4", (3,)), ("final", "<f4", (3,)),
                         ("light", "<i4"), ("lightDir_LightFrame", "<f4", (4,)), ("object", "<i4")])
assert RECORD_DTYPE.itemsize == 68


def build_oracle(tmpdir, src=SRC, name="libdoppler_oracle.so"):
    assert shutil.which("gcc") is not None, "gcc is needed to build tests/native/doppler_oracle.c"
    so = os.path.join(str(tmpdir), name)
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, src, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return bind(C.CDLL(so))


def bind(lib):
    """The entry points of doppler_oracle.c on any library that includes it (tests/native/aa_oracle.c's too)."""
    lib.rpt_doppler_oracle_render.restype = C.c_int
    lib.rpt_doppler_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.rpt_doppler_oracle_render_pinhole.restype = C.c_int
    lib.rpt_doppler_oracle_render_pinhole.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_int, C.c_void_p, C.c_int]
    lib.rpt_doppler_oracle_colour.restype = C.c_int
    lib.rpt_doppler_oracle_colour.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.rpt_doppler_oracle_record_bytes.restype = C.c_int
    assert lib.rpt_doppler_oracle_record_bytes() == RECORD_DTYPE.itemsize
    return lib


def render(lib, scene, W, H, flags, dirs=None, objects=None):
    """One frame of trace_doppler: (pixels[H W] 16 B, rgb[H, W, 3] float32, records[H, W] RECORD_DTYPE).  dirs: (H W, 3) float32
    unnormalised camera rays, None = the pinhole entry (createCamRay); objects: re-based objects of a turned camera, or None."""
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
    rec = np.zeros((H, W), dtype=RECORD_DTYPE)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    if dirs is None:
        rc = lib.rpt_doppler_oracle_render_pinhole(C.byref(a), int(flags), rec.ctypes.data, THREADS)
    else:
        assert dirs.shape == (W * H, 3) and dirs.dtype == np.float32 and dirs.flags.c_contiguous
        rc = lib.rpt_doppler_oracle_render(C.byref(a), dirs.ctypes.data, int(flags), rec.ctypes.data, THREADS)
    assert rc == 0
    return px, rgb, rec


def record11(rec):
    """The record's first 11 floats, (H, W, 11): the layout of rpt_set_debug_doppler."""
    return np.ascontiguousarray(rec).view(np.float32).reshape(rec.shape + (17,))[..., :11]


def colour(lib, D, rgb, flags):
    """The C S_f on D (n,), rgb (n, 3): (n, 3) float32."""
    D = np.asarray(D, dtype=np.float32)
    inp = np.empty((D.shape[0], 5), dtype=np.float32)
    inp[:, 0], inp[:, 1:4], inp[:, 4] = D, rgb, flags
    out = np.empty((D.shape[0], 3), dtype=np.float32)
    assert lib.rpt_doppler_oracle_colour(inp.ctypes.data, out.ctypes.data, D.shape[0]) == 0
    return out


def lens_dirs(W, H, v_fov=None):
    """(H W, 3) float32: the plane point the pinhole (v_fov None: s = 1) or the lens (s = tan(v_fov / 2)) normalises, in float32."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    s = np.float32(1.0) if v_fov is None else np.float32(math.tan(0.5 * float(np.float32(v_fov))))
    fx2 = (x / np.float32(W) - np.float32(0.5)) * (np.float32(W) / np.float32(H))
    fy2 = y / np.float32(H) - np.float32(0.5)
    return np.ascontiguousarray(np.stack([s * fx2, s * fy2, np.full_like(fx2, 0.5)], -1).reshape(-1, 3).astype(np.float32))


def pano_dirs(W, H, **kw):
    """(H W, 3) float32: the panorama's p from the library's own column and row tables."""
    from relativitypathtracer_amd.renderer import projection_tables
    cols, rows = projection_tables(W, H, **kw)
    sl, cl = cols[None, :, 0], cols[None, :, 1]
    sp, cp = rows[:, None, 0], rows[:, None, 1]
    p = np.stack([cp * sl, np.broadcast_to(sp, (H, W)), cp * cl], -1).astype(np.float32)
    return np.ascontiguousarray(p.reshape(-1, 3))
