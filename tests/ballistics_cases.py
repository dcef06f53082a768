"""The ballistic sets of the ballistic-pass tests and the ctypes face of tests/native/ballistics_oracle.c — TEST INFRASTRUCTURE shared by
tests/test_ballistics_model.py (no GPU: the C oracle against the float64 model, u = 0 against the particle oracle, and the non-vacuity of
the cases here on CPU event frames) and tests/test_gpu_ballistics.py (which runs exactly these on the device's own frames).  Scenes,
cameras, sizes and the view structure are tests/particles_cases.py's."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

import events_oracle as eo
import particles_cases as pc
from relativitypathtracer_amd import ballistics, particles
from relativitypathtracer_amd.events import _objects_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ballistics_oracle.c")

SIZES, CAMERAS, SCENES, MOTIONS, FLAGS, INTERVALS = pc.SIZES, pc.CAMERAS, pc.SCENES, pc.MOTIONS, pc.FLAGS, pc.INTERVALS
view = pc.view

# what each group of the particle cases' crafted set is given: (how it moves seen from the camera event, in the frame of its object, beta)
VELOCITIES = {"surface": ("across", 0.5), "near": ("towards", 0.8), "far": ("away", 0.8), "on pixels": ("rest", 0.0),
              "edges and corners": ("towards", 0.6), "outside": ("away", 0.3), "behind": ("across", 0.7), "seam": ("towards", 0.4),
              "poles": ("away", 0.6), "camera event": ("rest", 0.0), "pile": ("across", 0.9), "zero colour": ("towards", 0.2),
              "1e30": ("away", 0.99), "straddle": ("towards", 0.3), "lattice": ("across", 0.95)}
WINDOWED = "edges and corners"      # record i of this group: i % 3 == 0 a window around its emission time, 1 one that opens later, 2 one that has closed


def build_library(directory) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/ballistics_oracle.c")
    so = os.path.join(str(directory), "libballistics_oracle.so")
    p = subprocess.run(["gcc", *eo.CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_ballistics_oracle_place.restype = C.c_int
    lib.rpt_ballistics_oracle_place.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_ballistics_oracle_naive_tau.restype = C.c_int
    lib.rpt_ballistics_oracle_naive_tau.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_ballistics_oracle_pass.restype = C.c_int
    lib.rpt_ballistics_oracle_pass.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_thermal_oracle_x_green.restype = C.c_int
    lib.rpt_thermal_oracle_x_green.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


def x_green32(lib, kelvin) -> np.ndarray:
    """x_G per record as the host forms it from kelvin (tests/native/thermal_oracle.c)."""
    t = np.ascontiguousarray(kelvin, dtype=np.float32).reshape(-1)
    out = np.zeros(len(t), dtype=np.float32)
    assert lib.rpt_thermal_oracle_x_green(t.ctypes.data, len(t), out.ctypes.data) == 0
    return out


def _xg_ptr(xg, n):
    if xg is None:
        return None, None
    x = np.ascontiguousarray(xg, dtype=np.float32).reshape(-1)
    assert len(x) == n
    return x, x.ctypes.data


def oracle_place(lib, v, objects, bs, xg=None):
    """Rules 1-6 per record, float32 as the oracle computed them."""
    bs = np.ascontiguousarray(bs, dtype=ballistics.BALLISTIC_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    keep, xp = _xg_ptr(xg, len(bs))
    out = np.zeros((len(bs), 12), dtype=np.float32)
    assert lib.rpt_ballistics_oracle_place(C.byref(v), obj.ctypes.data, obj.size // 320, bs.ctypes.data, xp, len(bs), out.ctypes.data) == 0
    del keep
    return {"visible": out[:, 0] != 0, "X": out[:, 1], "Y": out[:, 2], "dist": out[:, 3], "rgb": out[:, 4:7], "D": out[:, 7], "te": out[:, 8],
            "r": out[:, 9], "a": out[:, 10], "tau": out[:, 11]}


def oracle_naive_tau(lib, objects, bs):
    """g (a - r') in float32 whatever the sign of a."""
    bs = np.ascontiguousarray(bs, dtype=ballistics.BALLISTIC_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    out = np.zeros(len(bs), dtype=np.float32)
    assert lib.rpt_ballistics_oracle_naive_tau(obj.ctypes.data, obj.size // 320, bs.ctypes.data, len(bs), out.ctypes.data) == 0
    return out


def oracle_pass(lib, v, objects, bs, pixels, records, xg=None):
    """Rules 1-7: (the framebuffer after the pass — a copy, all 16 bytes of every pixel —, (records seen, pixels changed))."""
    bs = np.ascontiguousarray(bs, dtype=ballistics.BALLISTIC_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    keep, xp = _xg_ptr(xg, len(bs))
    counts = (C.c_uint64 * 2)()
    assert lib.rpt_ballistics_oracle_pass(C.byref(v), obj.ctypes.data, obj.size // 320, bs.ctypes.data, xp, len(bs), out.ctypes.data, rec.ctypes.data, counts) == 0
    del keep
    return out, (int(counts[0]), int(counts[1]))


def without_negative_zero(ps):
    """The particle set with every -0.0 of pos made +0.0 (pos + beta * t keeps +0.0 and turns -0.0 into it)."""
    out = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE).copy()
    out["pos"] = out["pos"] + np.float32(0.0)
    assert not (np.signbit(out["pos"]) & (out["pos"] == 0)).any()
    return out


def from_particles(ps) -> np.ndarray:
    """The particle set as ballistic records at rest in their objects' frames, shining always."""
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    out = np.zeros(len(ps), dtype=ballistics.BALLISTIC_DTYPE)
    out["pos"], out["object"], out["rgb"] = ps["pos"], ps["object"], ps["rgb"]
    out["t0"], out["t1"] = -np.inf, np.inf
    return out


def moving(ps, groups, objects, camera, W, H, interval):
    """The particle set `ps` as ballistic records that PASS THROUGH the events the particles would be seen at: each group of `groups` with
    the velocity VELOCITIES gives it, pos backed out from the intended emission event (te, pos) of the float64 particle model, and the
    WINDOWED group on windows around, after and before its emission time."""
    ps = np.ascontiguousarray(ps, dtype=particles.PARTICLE_DTYPE)
    model = particles.project(ps, objects, camera, W, H, interval)
    cam = _objects_array(objects)["stationaryCam"][ps["object"]].astype(np.float64)
    pos = ps["pos"].astype(np.float64)
    w = pos - cam[:, 1:]
    r = np.linalg.norm(w, axis=1)
    with np.errstate(all="ignore"):
        away = np.where(r[:, None] > 0, w / r[:, None], 0.0)
    side = np.cross(away, (0.0, 1.0, 0.0))
    flat = np.linalg.norm(side, axis=1) < 1e-6
    side[flat] = np.cross(away[flat], (1.0, 0.0, 0.0))
    with np.errstate(all="ignore"):
        side = np.where(r[:, None] > 0, side / np.linalg.norm(side, axis=1, keepdims=True), 0.0)
    beta = np.zeros((len(ps), 3))
    for what, s in groups.items():
        how, b = VELOCITIES[what]
        beta[s] = {"rest": 0.0 * away[s], "towards": -b * away[s], "away": b * away[s], "across": b * side[s]}[how]
    te = model["te"]
    t0, t1 = np.full(len(ps), -np.inf), np.full(len(ps), np.inf)
    s = groups[WINDOWED]
    i = np.arange(s.stop - s.start)
    t0[s] = np.where(i % 3 == 0, te[s] - 0.5, np.where(i % 3 == 1, te[s] + 0.5, -np.inf))
    t1[s] = np.where(i % 3 == 0, te[s] + 0.5, np.where(i % 3 == 1, np.inf, te[s] - 0.5))
    return ballistics.from_arrays(pos, ps["object"], ps["rgb"].astype(np.float64), beta=beta, t0=t0, t1=t1, epoch=te)


def crafted(records, objects, camera, W, H, interval):
    """The crafted records of the parity test for one view, as (set, {what: slice}, bias): the particle cases' crafted set, built from
    that view's own records, set in motion."""
    ps, groups, bias = pc.crafted(records, objects, camera, W, H, interval)
    return moving(ps, groups, objects, camera, W, H, interval), groups, bias


def check_shows_something(lib, records, objects, camera, W, H, interval, bs, groups, bias, what):
    """What the parity test assumes of a case, asserted on the frame it runs on: pc.check_shows_something's asserts, and two more."""
    rec = np.ascontiguousarray(records).reshape(-1)
    place = oracle_place(lib, view(camera, W, H, interval, 0), objects, bs)
    t0, tb = pc.taps(place, rec, W, H, camera, 0.0), pc.taps(place, rec, W, H, camera, bias)
    assert (t0[:, 2] > 0).any(), f"{what}: no record in front of a hit pixel"
    assert (place["visible"] & (t0[:, 0] > t0[:, 1])).any(), f"{what}: no record hidden behind a hit pixel"
    assert (t0[:, 3] > 0).any(), f"{what}: no record over a miss pixel"
    full_sphere = camera.get("mode") == "equirect" and "h_fov" not in camera
    if not full_sphere:
        assert (place["visible"] & (t0[:, 0] == 0)).any(), f"{what}: no record outside the frame"
        assert (t0[groups["outside"], 0] == 0).all(), f"{what}: an `outside` record has a tap in the frame"
    s = groups["surface"]
    assert place["visible"][s].all() and (tb[s, 2] > 0).all(), f"{what}: a record on a surface is hidden in spite of the bias"
    assert (tb[:, 1] >= t0[:, 1]).all()
    assert (t0[groups["near"], 2] > 0).all(), f"{what}: a record pulled 1 % towards the camera is hidden"
    assert (t0[groups["far"], 0] > t0[groups["far"], 1]).all(), f"{what}: a record pushed 1 % away fails no depth test"
    assert not place["visible"][groups["camera event"]].any()
    if camera.get("mode", "pinhole") == "pinhole":
        assert not place["visible"][groups["behind"]].any()
    else:
        assert place["visible"][groups["seam"]].all() and place["visible"][groups["poles"]].all()
    assert "straddle" in groups, f"{what}: the frame has no 2 x 2 block across a silhouette edge"
    assert t0[groups["straddle"]].tolist() == [[4, 2, 0, 2]], f"{what}: the straddling record's taps {t0[groups['straddle']].tolist()}"
    # the two more: a record its own window skips — it shows once the window is opened —, and one on the receding branch
    opened = bs.copy()
    opened["t0"], opened["t1"] = -np.inf, np.inf
    free = oracle_place(lib, view(camera, W, H, interval, 0), objects, opened)
    s = groups[WINDOWED]
    shut = np.arange(s.stop - s.start) % 3 != 0
    assert not place["visible"][s][shut].any(), f"{what}: a record shows outside its window"
    assert (free["visible"][s][shut] & (pc.taps(free, rec, W, H, camera, 0.0)[s][shut, 1] > 0)).any(), f"{what}: no record is skipped by its window alone"
    assert np.array_equal(free["visible"][s][~shut], place["visible"][s][~shut]) and place["visible"][s][~shut].any()
    if interval == -1:
        assert (place["visible"] & (place["a"] > 0) & (t0[:, 1] > 0)).any(), f"{what}: no drawn record takes the a > 0 branch"
        assert (place["visible"] & (place["a"] <= 0) & (t0[:, 1] > 0)).any(), f"{what}: no drawn record takes the a <= 0 branch"
    return place, t0, tb
