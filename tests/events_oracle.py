"""tests/native/event_oracle.c built and bound with ctypes, and the per-pixel directions of the three cameras in their float32
operations — TEST INFRASTRUCTURE shared by tests/test_events_model.py (no GPU) and tests/test_gpu_events.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import oracle_ffi
from relativitypathtracer_amd.events import EVENT_DTYPE
from relativitypathtracer_amd.renderer import projection_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "event_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)
SHIPPED = ["cube", "arch", "bunny", "shadows", "cubes", "rulers", "ladder_paradox", "soccer"]      # every file of assets/reference/Scenes
SCENE_TIMES = {"cube": 0.0, "arch": 5.25, "bunny": 0.0, "shadows": 16.0, "cubes": 3.0, "rulers": 2.5, "ladder_paradox": 1.0, "soccer": 2.0}
CAMERAS = {"rest": (0.0, 0.0, 0.0), "0.9c": (0.0, 0.0, 0.9)}


def build_library(directory) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/event_oracle.c")
    so = os.path.join(str(directory), "libevent_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_event_oracle_render.restype = C.c_int
    lib.rpt_event_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_void_p, C.c_int]
    lib.rpt_event_oracle_sphere_dist.restype = C.c_int
    lib.rpt_event_oracle_sphere_dist.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def load_scene(name, camera="rest", interval=-1):
    from relativitypathtracer_amd import Scene
    s = Scene.from_file(name)
    s.set_interval(interval)
    # the moving camera passes the origin at t = 0: at the scenes' own times it would long have left them behind
    s.set_camera(CAMERAS[camera], SCENE_TIMES[name] if camera == "rest" else 0.0)
    s.update_objects()
    return s


def scene_from_text(text, v=(0.0, 0.0, 0.0), t=0.0, interval=None):
    from relativitypathtracer_amd import Scene
    s = Scene()
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


def pinhole_dirs(W, H, s=None):
    """The plane point createCamRay normalises, in its float32 operations; with a lens (s = (float)tan(v_fov / 2)) both plane
    coordinates times s, two more float products."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    fx = (x / np.float32(W) - np.float32(0.5)) * (np.float32(W) / np.float32(H))
    fy = y / np.float32(H) - np.float32(0.5)
    if s is not None:
        fx, fy = np.float32(s) * fx, np.float32(s) * fy
    return np.ascontiguousarray(np.stack([fx, fy, np.full_like(fx, 0.5)], -1).reshape(-1, 3).astype(np.float32))


def lens_scale(v_fov):
    """(float)tan((double)(float)v_fov / 2), as rpt_set_field_of_view forms it."""
    import math
    return np.float32(math.tan(float(np.float32(v_fov)) / 2.0))


def pano_dirs(W, H, **kw):
    cols, rows = projection_tables(W, H, **kw)
    sl, cl = cols[None, :, 0], cols[None, :, 1]
    sp, cp = rows[:, None, 0], rows[:, None, 1]
    p = np.stack([cp * sl, np.broadcast_to(sp, (H, W)), cp * cl], -1).astype(np.float32)
    return np.ascontiguousarray(p.reshape(-1, 3))


def oracle_args(scene, W, H, objects=None, interval=None):
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
    a.ambient, a.width, a.height, a.msaa = prm["ambient"], W, H, 1
    a.interval = prm["interval"] if interval is None else interval
    return a, keep


def oracle_events(lib, scene, W, H, dirs=None, objects=None, interval=None):
    """(H, W) records of EVENT_DTYPE from tests/native/event_oracle.c; dirs default to the pinhole's."""
    a, keep = oracle_args(scene, W, H, objects, interval)
    dirs = pinhole_dirs(W, H) if dirs is None else np.ascontiguousarray(dirs, dtype=np.float32)
    assert dirs.shape == (W * H, 3)
    out = np.zeros((H, W), dtype=EVENT_DTYPE)
    assert lib.rpt_event_oracle_render(C.byref(a), dirs.ctypes.data, out.ctypes.data, THREADS) == 0
    del keep
    return out


def null_cone_residual(events, objects):
    """The largest relative residual of |dx| = |dt| = dist over every hit record (none excluded), float64: max over pixels of
    max(| |dx| - dist |, | |dt| - dist |) / dist."""
    from relativitypathtracer_amd.events import camera_frame_events
    hit = events["object"] >= 0
    if not hit.any():
        return 0.0
    d = camera_frame_events(events, objects)[hit]
    dist = events["dist"][hit].astype(np.float64)
    space = np.sqrt((d[:, 1:] ** 2).sum(axis=1))
    res = np.maximum(np.abs(space - dist), np.abs(np.abs(d[:, 0]) - dist)) / dist
    return float(res.max())
