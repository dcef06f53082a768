"""Builds and binds tests/native/window_oracle.c — the CPU oracle with the per-object time windows of rpt_set_object_windows restated
(DESIGN.md "Time windows") — and chooses windows that act on a scene.  TEST INFRASTRUCTURE: used by tests/test_window_oracle.py (no GPU)
and tests/test_gpu_windows.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
import oracle_ffi
from relativitypathtracer_amd.events import EVENT_DTYPE, camera_frame_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "window_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)
HIT, BEHIND_REJECTED, SHADOW_REMOVED, LIGHT_OUT = 1, 2, 4, 8      # the bookkeeping byte of window_oracle.c


def build_library(directory) -> C.CDLL:
    assert shutil.which("gcc") is not None, "gcc is needed to build tests/native/window_oracle.c"
    so = os.path.join(str(directory), "libwindow_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_window_oracle_render.restype = C.c_int
    lib.rpt_window_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def render(lib, scene, W, H, windows=None, dirs=None, flags=0, objects=None, interval=None, sky=None, sky_frame=None):
    """One frame of trace_w: (pixels[H W] 16 B, rgb[H, W, 3] float32, events[H, W] EVENT_DTYPE, book[H, W] uint8).  windows: (n, 2) float32
    or None (every test accepts); dirs: (H W, 3) float32 unnormalised camera rays, default the pinhole's; flags: the Doppler flags; objects:
    re-based objects of a turned camera; sky: an (h, w, 3) uint8 image with sky_frame its 4 x 4 float32 matrix."""
    a, keep = eo.oracle_args(scene, W, H, objects, interval)
    dirs = eo.pinhole_dirs(W, H) if dirs is None else np.ascontiguousarray(dirs, dtype=np.float32)
    assert dirs.shape == (W * H, 3)
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    ev = np.zeros((H, W), dtype=EVENT_DTYPE)
    book = np.zeros((H, W), dtype=np.uint8)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    w = None
    if windows is not None:
        w = np.ascontiguousarray(windows, dtype=np.float32)
        assert w.shape == (a.object_count, 2)
    img = E = None
    if sky is not None:
        img = np.ascontiguousarray(sky, dtype=np.uint8)
        E = np.ascontiguousarray(np.eye(4) if sky_frame is None else sky_frame, dtype=np.float32)
    rc = lib.rpt_window_oracle_render(C.byref(a), dirs.ctypes.data, None if w is None else w.ctypes.data, int(flags),
                                      None if E is None else E.ctypes.data, None if img is None else img.ctypes.data,
                                      0 if img is None else img.shape[1], 0 if img is None else img.shape[0], ev.ctypes.data, book.ctypes.data, THREADS)
    assert rc == 0
    del keep
    return px, rgb, ev, book


def default_windows(n):
    w = np.empty((n, 2), dtype=np.float32)
    w[:, 0], w[:, 1] = -np.inf, np.inf
    return w


def accepts(windows, objects, t):
    """in(W[object], t) of DESIGN.md "Time windows", elementwise in float32."""
    w = np.asarray(windows, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    return ~(t < w[objects, 0]) & ~(t >= w[objects, 1])


def light_emission_times(events, objs, light, interval):
    """For every hit pixel the emission time, in light `light`'s rest frame, of the light that reaches the hit point (rule 3's tl up to
    rounding and the 0.001 offset along the normal): float64, NaN on a miss.  Used to place a window's bound only, never to judge a frame."""
    cam = camera_frame_events(events, objs)                         # displacement from the camera event, camera frame
    o = objs[light]
    L = o["Lorentz"].astype(np.float64)
    p = cam @ L.T + o["stationaryCam"].astype(np.float64)           # the hit event in the light's rest frame
    pos = o["M"].astype(np.float64)[:3, 3]
    return p[..., 0] + interval * np.linalg.norm(pos - p[..., 1:], axis=-1)


def choose_windows(lib, scene, W, H, dirs=None, objects=None, interval=None, min_pixels=12, flip=False):
    """Windows that act (the issue's rule): from the CPU event frame WITHOUT windows, every object with at least min_pixels visible
    pixels gets one bound at the median emission time of those pixels — alternately the lower bound (the object begins) and the upper one
    (it ends), in the order of the object list; a light gets its lower bound at the first quartile, over all hit pixels, of the time its
    light left it, so that it is dark for about a quarter of them (the farthest).  flip swaps the alternation."""
    objs = scene.objects() if objects is None else np.ascontiguousarray(objects).view(np.uint8).reshape(-1).view(scene.objects().dtype)
    itv = scene.params["interval"] if interval is None else interval
    ev = render(lib, scene, W, H, None, dirs=dirs, objects=objects, interval=interval)[2]
    w = default_windows(len(objs))
    k = 1 if flip else 0
    for i in range(len(objs)):
        if objs[i]["light"] and itv != 0:
            tl = light_emission_times(ev, objs, i, itv)
            lit = (ev["object"] >= 0) & (ev["object"] != i)
            if lit.sum() >= min_pixels:
                w[i, 0] = np.float32(np.quantile(tl[lit], 0.25))
            continue
        seen = ev["object"] == i
        if seen.sum() < min_pixels:
            continue
        m = np.float32(np.median(ev["event"][..., 0][seen]))
        w[i, k & 1] = m
        k += 1
    return w


def many_objects_text():
    """66 objects, so that objects 64 and 65 lie beyond the 64-bit object mask: a light, 63 small spheres in a grid (a third of them
    moving each way), and LAST the floor (64) and a large moving sphere in front of the grid (65), both prominent in the frame."""
    lines = ["Os p0,6,9,0,0,1,0,0.2,0.2,0.2 l1 c5,5,5"]
    motions = ["", " v0.3,0,0", " v-0.5,0,0.2"]
    for k in range(63):
        x, y = -7.0 + 2.0 * (k % 8), -3.0 + 1.0 * (k // 8)
        lines.append(f"Os p{x},{y},12,0,0,1,0,0.45,0.45,0.45 c{0.3 + 0.1 * (k % 7)},{0.9 - 0.1 * (k % 5)},0.5{motions[k % 3]}")
    lines.append("Oc p0,-4,10,0,0,1,0,12,0.5,12 c1,1,1")
    lines.append("Os p-1,-1,9,0,0,1,0,1.5,1.5,1.5 c0.2,0.9,0.3 v0.4,0,0")
    return "\n".join(lines) + "\nA0.2\nW2,2,2\nR\n"


def many_objects_scene(t=2.0):
    s = eo.scene_from_text(many_objects_text(), t=t)
    assert len(s.objects()) == 66
    return s


# cubes.txt and rulers.txt have no light, so rules 2 and 3 could never act on them, and the rulers never overlap on the screen.  The
# windowed tests use them with a light and a surface that takes shadows ADDED (the files' own objects, textures and motions untouched):
# cubes gets a lamp above and a floor below its two rows; rulers a lamp beside the camera and a wall behind the rulers, at camera time
# 10, when both rulers are in view.  rulers.txt sets interval 0 itself (its `I`): "rulers" keeps that, "rulers_delay" is the same scene
# with light delay on.
LIT = {
    "cubes": "Os p-5,6,6,0,0,1,0,0.3,0.3,0.3 l1 c8,8,8\nOc p-5,-3,9,0,0,1,0,14,0.5,14 c1,1,1\nA0.2",
    "rulers": "Os p0,2,1,0,0,1,0,0.1,0.1,0.1 l1 c5,5,5\nOc p0,0,9,0,0,1,0,12,8,0.5 c1,1,1\nA0.2",
}
RULERS_TIME = 10.0

# which way choose_windows alternates per test scene: chosen on the CPU reference alone so that tests/test_window_oracle.py's
# non-vacuity conditions hold (in "many" the big sphere, object 65, must BEGIN for its shadow on the floor to be removed; in
# "rulers_delay" the rulers' shadows on the wall likewise)
FLIP = {"many": True, "rulers_delay": True}
SCENES = ("arch", "shadows", "cubes", "rulers", "rulers_delay", "many")


def lit_scene(name, v, t, interval):
    """Scenes/<name>.txt with LIT[name]'s objects appended (its `I`, if any, replaced by `interval`)"""
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.scene import ASSET_ROOT
    with open(os.path.join(ASSET_ROOT, "Scenes", name + ".txt")) as f:
        lines = [line for line in f.read().splitlines() if line.strip() not in ("R", "I")]
    s = Scene()
    s.inputScene("\n".join(lines) + "\n" + LIT[name] + "\nR\n")
    s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


def load(name):
    """A windowed test scene by name: "arch", "shadows" (conftest.CONFIGS as they are), "cubes" (its configuration, lit), "rulers"
    (lit, interval 0 as the file says), "rulers_delay" (the same with light delay on), "many" (generated, 66 objects)."""
    from conftest import CONFIGS, load_config
    if name == "many":
        return many_objects_scene()
    if name == "cubes":
        return lit_scene("cubes", CONFIGS["cubes"]["v"], CONFIGS["cubes"]["t"], -1)
    if name in ("rulers", "rulers_delay"):
        return lit_scene("rulers", (0.0, 0.0, 0.0), RULERS_TIME, 0 if name == "rulers" else -1)
    return load_config(name)
