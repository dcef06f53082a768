"""The scenes, cameras, sizes and particle sets of the particle-pass tests, and the ctypes face of tests/native/particles_oracle.c — TEST
INFRASTRUCTURE shared by tests/test_particles_model.py (no GPU: the C oracle against the float64 model, and the non-vacuity of the cases
here on CPU event frames) and tests/test_gpu_particles.py (which runs exactly these on the device's own frames)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
import stars_cases as sc
from relativitypathtracer_amd import particles, worldline
from relativitypathtracer_amd.events import _objects_array
from relativitypathtracer_amd.renderer import orient_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "particles_oracle.c")

SIZES = sc.SIZES                             # 128 x 72 and 67 x 41 (a ragged last workgroup in both kernels)
CAMERAS = sc.CAMERAS                         # pinhole, the lens turned by YPR, the full sphere, a partial panorama
SCENES = ["cubes", "arch"]
MOTIONS = ["rest", "0.9c"]
FLAGS = [0, 1, 2, 3]
INTERVALS = [-1, 0]
BIAS = 1e-3                                  # times the largest dist of the particles on surfaces


class ParticlesView(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("interval", C.c_int), ("doppler", C.c_int), ("camera", C.c_int),
                ("inverse_square", C.c_int), ("depth_bias", C.c_float), ("lens_scale", C.c_float), ("h_fov", C.c_float),
                ("v_fov", C.c_float), ("yaw", C.c_float), ("white_point", C.c_float * 3)]


def build_library(directory) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/particles_oracle.c")
    so = os.path.join(str(directory), "libparticles_oracle.so")
    p = subprocess.run(["gcc", *eo.CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_particles_oracle_place.restype = C.c_int
    lib.rpt_particles_oracle_place.argtypes = [C.POINTER(ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_particles_oracle_pass.restype = C.c_int
    lib.rpt_particles_oracle_pass.argtypes = [C.POINTER(ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def view(camera, W, H, interval, flags, white_point=(1.0, 1.0, 1.0), inverse_square=False, depth_bias=0.0) -> ParticlesView:
    v = ParticlesView()
    v.width, v.height, v.interval, v.doppler = W, H, interval, flags
    v.camera = 1 if camera.get("mode", "pinhole") == "equirect" else 0
    v.inverse_square, v.depth_bias = int(bool(inverse_square)), depth_bias
    v.lens_scale = float(eo.lens_scale(camera["v_fov"])) if v.camera == 0 and camera.get("v_fov") else 1.0
    v.h_fov, v.v_fov, v.yaw = camera.get("h_fov", 2.0 * math.pi), camera.get("v_fov", math.pi), camera.get("yaw", 0.0)
    v.white_point[:] = white_point
    return v


def scene_objects(scene, camera) -> np.ndarray:
    """The Object[] a context renders `scene` with under one of CAMERAS: (n, 320) uint8, re-based when the camera is turned."""
    ypr = camera.get("orientation")
    if ypr is None:
        return np.ascontiguousarray(_objects_array(scene)).view(np.uint8).reshape(-1, 320).copy()
    return orient_objects(scene, *ypr)


def _windows_ptr(windows):
    if windows is None:
        return None, None
    w = np.ascontiguousarray(windows, dtype=np.float32).reshape(-1)
    return w, w.ctypes.data


def oracle_place(lib, v, objects, ps, windows=None):
    """Rules 1-4 per particle, float32 as the oracle computed them."""
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    keep, wp = _windows_ptr(windows)
    out = np.zeros((len(ps), 10), dtype=np.float32)
    assert lib.rpt_particles_oracle_place(C.byref(v), obj.ctypes.data, obj.size // 320, wp, ps.ctypes.data, len(ps), out.ctypes.data) == 0
    del keep
    return {"visible": out[:, 0] != 0, "X": out[:, 1], "Y": out[:, 2], "dist": out[:, 3], "rgb": out[:, 4:7], "D": out[:, 7], "te": out[:, 8], "r": out[:, 9]}


def oracle_pass(lib, v, objects, ps, pixels, records, windows=None):
    """Rules 1-6: (the framebuffer after the pass — a copy, all 16 bytes of every pixel —, (particles seen, pixels changed))."""
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    keep, wp = _windows_ptr(windows)
    counts = (C.c_uint64 * 2)()
    assert lib.rpt_particles_oracle_pass(C.byref(v), obj.ctypes.data, obj.size // 320, wp, ps.ctypes.data, len(ps), out.ctypes.data, rec.ctypes.data, counts) == 0
    del keep
    return out, (int(counts[0]), int(counts[1]))


def rest_position(objects, o, n, d, interval):
    """Where, in the rest frame of object o, a point sits that the camera sees in the direction n (camera frame, (..., 3), float64) at
    the camera-frame distance d: the displacement (-d, d n) on the past light cone (interval -1) or (0, d n) on the simultaneity slice
    (interval 0), through the object's Lorentz, from stationaryCam."""
    objs = _objects_array(objects)
    n = np.asarray(n, dtype=np.float64).reshape(-1, 3)
    d = np.broadcast_to(np.asarray(d, dtype=np.float64), (len(n),))
    k = np.concatenate([(-d if interval == -1 else 0.0 * d)[:, None], n * d[:, None]], axis=1)
    w = k @ objs["Lorentz"][o].astype(np.float64).reshape(4, 4).T
    return objs["stationaryCam"][o].astype(np.float64).reshape(4)[1:] + w[:, 1:]


def taps(place, records, W, H, camera, depth_bias=0.0):
    """Rule 5's tests per particle in numpy, from a place() or project() result: (taps inside the frame, taps that pass the depth test,
    passing taps over a hit pixel, passing taps over a miss pixel) — (N, 4) ints; all zero for a skipped particle."""
    rec = np.asarray(records).reshape(-1)
    wrap = camera.get("mode", "pinhole") == "equirect" and np.float32(camera.get("h_fov", 2.0 * math.pi)) == np.float32(2.0 * math.pi)
    out = np.zeros((len(place["X"]), 4), dtype=np.int64)
    for i in np.nonzero(place["visible"])[0]:
        x0, y0 = int(math.floor(place["X"][i])), int(math.floor(place["Y"][i]))
        for k in range(4):
            x, y = x0 + (k & 1), y0 + (k >> 1)
            if wrap:
                x = x + W if x < 0 else (x - W if x >= W else x)
            if x < 0 or x >= W or y < 0 or y >= H:
                continue
            out[i, 0] += 1
            r = rec[y * W + x]
            if r["object"] < 0 or np.float32(place["dist"][i]) - np.float32(depth_bias) < r["dist"]:
                out[i, 1] += 1
                out[i, 2 if r["object"] >= 0 else 3] += 1
    return out


def silhouette_block(records, W, H):
    """(x, y, hit column) of a 2 x 2 block of pixels with one column hit and the other missed in both rows, away from the frame's edge;
    None if the frame has none."""
    hit = (np.asarray(records)["object"] >= 0).reshape(H, W)
    for y in range(2, H - 3):
        for x in range(2, W - 3):
            a, b = hit[y:y + 2, x], hit[y:y + 2, x + 1]
            if a.all() and not b.any():
                return x, y, 0
            if b.all() and not a.any():
                return x, y, 1
    return None


def crafted(records, objects, camera, W, H, interval):
    """The crafted particles of the parity test for one view, as (set, {what: slice}, bias), built from that view's own records."""
    rec = np.ascontiguousarray(records).reshape(-1)
    objs = _objects_array(objects)
    hit = rec["object"] >= 0
    assert hit.any() and (~hit).any()
    groups, parts = {}, []
    count = [0]

    def add(what, ps):
        groups[what] = slice(count[0], count[0] + len(ps))
        count[0] += len(ps)
        parts.append(ps)

    def scaled(ps, f):       # the same points at f times their distance from the camera event, along the same line of sight
        cam = objs["stationaryCam"][ps["object"]].astype(np.float64)[:, 1:]
        out = ps.copy()
        out["pos"] = cam + (ps["pos"].astype(np.float64) - cam) * f
        return out

    panorama = camera.get("mode", "pinhole") == "equirect"
    # (sc.pixel_direction(x, y) is the direction the pass projects to X = x, Y = y, for the pinhole and for the panorama alike)
    surface = particles.at_events(rec, (0.9, 0.5, 0.2), stride=max(1, int(hit.sum()) // 300))
    add("surface", surface)
    add("near", scaled(surface, 0.99))
    add("far", scaled(surface, 1.01))
    near_d = 0.5 * float(rec["dist"][hit].min())                    # in front of everything the frame sees
    o = int(rec["object"][hit][0])

    def at_pixels(xs, ys, d, rgb, obj=o):
        n = sc.pixel_direction(camera, W, H, np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64))
        return particles.from_arrays(rest_position(objects, obj, n, d, interval), obj, rgb)

    def along(dirs, d, rgb):
        n = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
        return particles.from_arrays(rest_position(objects, o, n / np.linalg.norm(n, axis=1, keepdims=True), d, interval), o, rgb)

    add("on pixels", at_pixels([3, W // 2, W - 4, W // 3, 1], [2, H // 2, H - 3, 2 * H // 3, H - 2], near_d, (0.8, 0.6, 0.4)))
    # (the last two: exactly one pixel outside — the inner taps are in the frame with weight 0)
    xs = [0, W - 1, 0, W - 1, W // 2, W // 2, 0, W - 1, -0.5, W - 0.5, W // 2, W // 2, -1.0, W // 2]
    ys = [0, 0, H - 1, H - 1, 0, H - 1, H // 2, H // 2, H // 2, H // 2, -0.5, H - 0.5, H // 2, -1.0]
    add("edges and corners", at_pixels(xs, ys, near_d, (0.5, 0.9, 0.7)))
    if not panorama:
        add("outside", at_pixels([-2.5, W + 1.5, W // 2, W // 2], [H // 2, H // 2, -2.5, H + 1.5], near_d, (1.0, 1.0, 1.0)))
    else:       # (the full sphere has no outside: every direction has a tap in the frame; a partial one has)
        yaw = float(camera.get("yaw", 0.0))
        add("outside", along([(math.sin(yaw + 3.1), 0.0, math.cos(yaw + 3.1)), (0.0, 1.0, 1e-3)], near_d, (1.0, 1.0, 1.0)))
    add("behind", along([(0.1, 0.1, -1.0), (0.0, 0.0, -1.0), (1.0, 0.0, -0.2), (0.0, 1.0, -0.05)], near_d, (1.0, 1.0, 1.0)))
    yaw = float(camera.get("yaw", 0.0)) if panorama else 0.0
    add("seam", along([(math.sin(yaw + math.pi), 0.0, math.cos(yaw + math.pi)), (math.sin(yaw + math.pi - 1e-7), 0.1, math.cos(yaw + math.pi - 1e-7)),
                       (math.sin(yaw - math.pi + 1e-3), -0.2, math.cos(yaw - math.pi + 1e-3))], near_d, (0.9, 0.9, 0.2)))
    add("poles", along([(0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (1e-4, 1.0, 1e-4), (-1e-5, -1.0, 1e-5)], near_d, (0.3, 0.6, 0.9)))
    add("camera event", particles.from_arrays(objs["stationaryCam"][o].astype(np.float64).reshape(4)[None, 1:], o, (1.0, 1.0, 1.0)))
    miss = np.nonzero(~hit.reshape(H, W)[2:H - 2, 2:W - 2])
    pile = (int(miss[1][0]) + 2, int(miss[0][0]) + 2)
    add("pile", at_pixels(np.full(1000, pile[0] + 0.25), np.full(1000, pile[1] + 0.25), near_d, (90.0, 70.0, 0.004)))
    add("zero colour", at_pixels([7.0], [5.0], near_d, (0.0, 0.0, 0.0)))
    add("1e30", at_pixels([9.3], [6.6], near_d, (1e30, 1e30, 1e30)))
    block = silhouette_block(rec, W, H)
    if block is not None:       # behind the surface of the block's hit column, over the gap between its two columns and two rows
        x, y, column = block
        behind = 1.05 * float(rec["dist"].reshape(H, W)[y:y + 2, x + column].max())
        add("straddle", at_pixels([x + 0.5], [y + 0.5], behind, (0.7, 0.7, 0.7), int(rec["object"].reshape(H, W)[y, x + column])))
    # a lattice of lamps riding the first object the frame sees, around the first point of it that the frame sees
    centre = surface["pos"][surface["object"] == o][0].astype(np.float64)
    add("lattice", particles.lattice(o, centre - 0.6, centre + 0.6, 4, (0.4, 0.4, 0.9)))
    ps = np.concatenate(parts)
    assert len(ps) <= 4096
    bias = BIAS * float(rec["dist"][hit].max())
    return ps, groups, bias


def check_shows_something(lib, records, objects, camera, W, H, interval, ps, groups, bias, what):
    """What the parity test assumes of a case, asserted on the frame it runs on."""
    rec = np.ascontiguousarray(records).reshape(-1)
    place = oracle_place(lib, view(camera, W, H, interval, 0), objects, ps)
    t0, tb = taps(place, rec, W, H, camera, 0.0), taps(place, rec, W, H, camera, bias)
    assert (t0[:, 2] > 0).any(), f"{what}: no particle in front of a hit pixel"
    assert (place["visible"] & (t0[:, 0] > t0[:, 1])).any(), f"{what}: no particle hidden behind a hit pixel"
    assert (t0[:, 3] > 0).any(), f"{what}: no particle over a miss pixel"
    full_sphere = camera.get("mode") == "equirect" and "h_fov" not in camera
    if not full_sphere:
        assert (place["visible"] & (t0[:, 0] == 0)).any(), f"{what}: no particle outside the frame"
        assert (t0[groups["outside"], 0] == 0).all(), f"{what}: an `outside` particle has a tap in the frame"
    s = groups["surface"]
    assert place["visible"][s].all() and (tb[s, 2] > 0).all(), f"{what}: a particle on a surface is hidden in spite of the bias"
    assert (tb[:, 1] >= t0[:, 1]).all()
    assert (t0[groups["near"], 2] > 0).all(), f"{what}: a particle pulled 1 % towards the camera is hidden"
    assert (t0[groups["far"], 0] > t0[groups["far"], 1]).all(), f"{what}: a particle pushed 1 % away fails no depth test"
    assert not place["visible"][groups["camera event"]].any()
    if camera.get("mode", "pinhole") == "pinhole":
        assert not place["visible"][groups["behind"]].any()
    else:
        assert place["visible"][groups["seam"]].all() and place["visible"][groups["poles"]].all()
    assert "straddle" in groups, f"{what}: the frame has no 2 x 2 block across a silhouette edge"
    assert t0[groups["straddle"]].tolist() == [[4, 2, 0, 2]], f"{what}: the straddling particle's taps {t0[groups['straddle']].tolist()}"
    return place, t0, tb


# ---- the windowed case: a body of three legs (worldline.piecewise) with lamps riding every leg -----------------------------------
def turnaround():
    """(worldline, scene, particle set): a cube that goes out along +x, turns, comes back and leaves upwards — three legs, objects 0, 1
    and 2 — and a sphere at rest behind; 3 x 3 x 1 lamps ride every leg, in the plane in front of the cube.  At the camera time the
    light of more than one leg's lamps is on its way: without the windows they show all at once."""
    wl = worldline.piecewise([(0.0, -3.0, 0.0, 4.0), (5.0, 0.0, 0.0, 4.0), (10.0, -3.0, 0.0, 4.0), (15.0, -3.0, 2.0, 4.0)])
    text = wl.to_dsl("Oc", scale=(1.0, 0.6, 0.4), extra="c0.3,0.5,0.9") + "Os p1.5,1.2,6,0,0,1,0,0.4,0.4,0.4 c0.9,0.6,0.2\nR\n"
    scene = eo.scene_from_text(text, t=9.0)
    sets = []
    for j, leg in enumerate(wl):
        p = np.asarray(leg.position, dtype=np.float64)
        sets.append(particles.lattice(j, p + (-0.8, -0.5, -0.6), p + (0.8, 0.5, -0.6), (3, 3, 1), ((0.9, 0.2, 0.2), (0.2, 0.9, 0.2), (0.2, 0.2, 0.9))[j]))
    return wl, scene, np.concatenate(sets)
