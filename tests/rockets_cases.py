"""The rocket sets of the rocket-pass tests and the ctypes face of tests/native/rockets_oracle.c — TEST INFRASTRUCTURE shared by
tests/test_rockets_model.py (no GPU: the C oracle against the float64 model, and the non-vacuity of the cases here on CPU event frames)
and tests/test_gpu_rockets.py (which runs exactly these on the device's own frames).  Scenes, cameras, sizes and the view structure are
tests/particles_cases.py's; the set is tests/ballistics_cases.py's crafted one with accelerations laid over it.

A record of the ballistic set is seen at one event of its straight worldline, with one velocity there.  The rocket made from it passes
through the same event with the same velocity and accelerates: it is seen at that event — a timelike worldline meets a past light cone
once — in the same place, at the same depth and with the same Doppler factor, to rounding; so what the ballistic cases assume of a frame
(a record in front of a hit pixel, one hidden, one on a surface that the bias lets through, ...) holds of the rockets too."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import ballistics_cases as bc
import events_oracle as eo
import particles_cases as pc
from relativitypathtracer_amd import ballistics, rockets
from relativitypathtracer_amd.events import _objects_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "rockets_oracle.c")

SIZES, CAMERAS, SCENES, MOTIONS, FLAGS, INTERVALS = pc.SIZES, pc.CAMERAS, pc.SCENES, pc.MOTIONS, pc.FLAGS, pc.INTERVALS
view = pc.view

# record i of the ballistic set gets the acceleration of class i % 3: none, gentle (alpha |w| = 1e-2, |w| the light's way from the
# emission event in the object's frame), strong (alpha |w| = 1); then two groups of their own
ACCELERATIONS = ("none", "gentle", "strong")
ALPHA_W = {"none": 0.0, "gentle": 1e-2, "strong": 1.0}
FAST = 64           # records at gamma 2 .. 30, coming and going, i % 2
HORIZON = 24        # records of each of rule 5's two skips
BRANCH_MIN = 20     # what every branch of rule 5 must hold in every case


def build_library(directory) -> C.CDLL:
    if shutil.which("gcc") is None:
        raise RuntimeError("gcc is needed to build tests/native/rockets_oracle.c")
    so = os.path.join(str(directory), "librockets_oracle.so")
    p = subprocess.run(["gcc", *eo.CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_rockets_oracle_place.restype = C.c_int
    lib.rpt_rockets_oracle_place.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.rpt_rockets_oracle_pass.restype = C.c_int
    lib.rpt_rockets_oracle_pass.argtypes = [C.POINTER(pc.ParticlesView), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.rpt_thermal_oracle_x_green.restype = C.c_int
    lib.rpt_thermal_oracle_x_green.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return lib


x_green32 = bc.x_green32


def oracle_place(lib, v, objects, rs, xg=None):
    """Rules 1-6 per record, float32 as the oracle computed them."""
    rs = np.ascontiguousarray(rs, dtype=rockets.ROCKET_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    keep, xp = bc._xg_ptr(xg, len(rs))
    out = np.zeros((len(rs), 16), dtype=np.float32)
    assert lib.rpt_rockets_oracle_place(C.byref(v), obj.ctypes.data, obj.size // 320, rs.ctypes.data, xp, len(rs), out.ctypes.data) == 0
    del keep
    return {"visible": out[:, 0] != 0, "X": out[:, 1], "Y": out[:, 2], "dist": out[:, 3], "rgb": out[:, 4:7], "D": out[:, 7], "te": out[:, 8],
            "r": out[:, 9], "nq": out[:, 10], "tau": out[:, 11], "Aq": out[:, 12], "z": out[:, 13], "d": out[:, 14], "branch": out[:, 15].astype(np.int64)}


def oracle_pass(lib, v, objects, rs, pixels, records, xg=None):
    """Rules 1-7: (the framebuffer after the pass — a copy, all 16 bytes of every pixel —, (records seen, pixels changed))."""
    rs = np.ascontiguousarray(rs, dtype=rockets.ROCKET_DTYPE)
    obj = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    out = np.ascontiguousarray(pixels).copy()
    rec = np.ascontiguousarray(records)
    assert out.nbytes == 16 * v.width * v.height and rec.nbytes == 32 * v.width * v.height
    keep, xp = bc._xg_ptr(xg, len(rs))
    counts = (C.c_uint64 * 2)()
    assert lib.rpt_rockets_oracle_pass(C.byref(v), obj.ctypes.data, obj.size // 320, rs.ctypes.data, xp, len(rs), out.ctypes.data, rec.ctypes.data, counts) == 0
    del keep
    return out, (int(counts[0]), int(counts[1]))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def accelerated(bs, objects, camera, W, H, interval, rng):
    """The ballistic set `bs` as rockets through the events the ballistic records are seen at, with their velocities there, record i
    under the acceleration of class ACCELERATIONS[i % 3] in a direction of its own."""
    model = ballistics.project(bs, objects, camera, W, H, interval)
    way = np.abs(model["tau"]) if interval == -1 else np.linalg.norm(model["pos_e"] - _objects_array(objects)["stationaryCam"][bs["object"]].astype(np.float64)[:, 1:], axis=1)
    way = np.where(np.isfinite(way) & (way > 0.0), way, 1.0)
    alpha = np.array([ALPHA_W[ACCELERATIONS[i % 3]] for i in range(len(bs))]) / way
    ok = np.isfinite(model["pos_e"]).all(axis=1) & np.isfinite(model["te"])      # (a record with no event keeps its place at time 0)
    return rockets.from_arrays(np.where(ok[:, None], model["pos_e"], bs["pos"].astype(np.float64)), bs["object"], bs["rgb"].astype(np.float64),
                               u=bs["u"].astype(np.float64), acc=alpha[:, None] * _unit(rng, len(bs)), t0=bs["t0"].astype(np.float64),
                               t1=bs["t1"].astype(np.float64), epoch=np.where(ok, model["te"], 0.0))


def fast(bs, groups, objects, camera, W, H, interval, rng):
    """FAST rockets through the events the lattice of the ballistic set is seen at, at gamma 2 .. 30 straight towards the camera event
    (even records) and straight away from it (odd ones), speeding up or slowing down along their way with alpha |w| = 0.1."""
    some = bs[groups["lattice"]][:FAST]
    model = ballistics.project(some, objects, camera, W, H, interval)
    cam = _objects_array(objects)["stationaryCam"][some["object"]].astype(np.float64)
    away = model["pos_e"] - cam[:, 1:]
    way = np.linalg.norm(away, axis=1)
    away = away / way[:, None]
    gamma = np.linspace(2.0, 30.0, len(some))
    sign = np.where(np.arange(len(some)) % 2 == 0, -1.0, 1.0)
    u = (sign * np.sqrt(gamma * gamma - 1.0))[:, None] * away
    acc = (0.1 / way * np.where(np.arange(len(some)) % 4 < 2, 1.0, -1.0))[:, None] * away
    return rockets.from_arrays(model["pos_e"], some["object"], (0.6, 0.8, 1.0), u=u, acc=acc, epoch=model["te"])


def beyond_the_horizon(objects, o, near_d, rng):
    """HORIZON rockets of each of rule 5's two skips (none: Aq >= 0 with n <= 0; a root with d <= 0), found among random states at the
    camera's time in the frame of object o — some near_d from the camera event, proper velocities up to 3, alpha |w| from 1.5 to 8 — and
    kept where the float64 model decides with a margin.  The camera's past light cone never meets them."""
    cam = _objects_array(objects)["stationaryCam"][o].astype(np.float64).reshape(4)
    n = 4000
    w0 = _unit(rng, n) * (near_d * rng.uniform(0.5, 2.0, n))[:, None]
    u1 = _unit(rng, n) * rng.uniform(0.0, 3.0, n)[:, None]
    acc = _unit(rng, n) * (rng.uniform(1.5, 8.0, n) / np.linalg.norm(w0, axis=1))[:, None]
    frame = {"InvLorentz": np.eye(4)[None], "stationaryCam": np.array([[0.0, 0.0, 0.0, 0.0]])}      # the state IS at the camera's time
    zero = np.zeros(n, dtype=np.int64)
    m = rockets.project_columns(w0, zero, np.ones((n, 3)), u1, acc, np.full(n, -np.inf), np.full(n, np.inf), frame, dict(mode="equirect"), 64, 32, -1)
    al2 = (acc * acc).sum(axis=1)
    none = (m["branch"] == 2) & (m["Aq"] > 0.05 * (1.0 + 0.25 * al2 * (w0 * w0).sum(axis=1))) & (m["nq"] < -0.05 * np.linalg.norm(u1, axis=1) * np.linalg.norm(w0, axis=1))
    late = (m["branch"] == 3) & (m["d"] < -0.05) & (np.abs(m["nq"]) > 0.05 * np.linalg.norm(u1, axis=1) * np.linalg.norm(w0, axis=1)) & (np.abs(m["Aq"]) > 0.05)
    assert none.sum() >= HORIZON and late.sum() >= HORIZON, (int(none.sum()), int(late.sum()))
    keep = np.r_[np.nonzero(none)[0][:HORIZON], np.nonzero(late)[0][:HORIZON]]
    return rockets.from_arrays(cam[1:] + w0[keep], o, (1.0, 1.0, 1.0), u=u1[keep], acc=acc[keep], epoch=cam[0])


def crafted(records, objects, camera, W, H, interval):
    """The crafted records of the parity test for one view, as (set, {what: slice}, bias): the ballistic cases' crafted set, built from
    that view's own records, with accelerations laid over it — groups as there, every third record with none, a gentle, a strong one —,
    and the groups "fast" and "horizon" behind it."""
    bs, groups, bias = bc.crafted(records, objects, camera, W, H, interval)
    rng = np.random.default_rng(25)
    rec = np.ascontiguousarray(records).reshape(-1)
    hit = rec["object"] >= 0
    parts = [accelerated(bs, objects, camera, W, H, interval, rng), fast(bs, groups, objects, camera, W, H, interval, rng),
             beyond_the_horizon(objects, int(rec["object"][hit][0]), 0.5 * float(rec["dist"][hit].min()), rng)]
    groups = dict(groups)
    at = len(bs)
    for what, part in zip(("fast", "horizon"), parts[1:]):
        groups[what] = slice(at, at + len(part))
        at += len(part)
    rs = np.concatenate(parts)
    assert len(rs) <= 4096
    return rs, groups, bias


def check_shows_something(lib, records, objects, camera, W, H, interval, rs, groups, bias, what):
    """What the parity test assumes of a case, asserted on the frame it runs on: the float64 model decides the branches of rule 5 —
    light-cone quantities, whatever the view's interval —, the oracle the taps."""
    rec = np.ascontiguousarray(records).reshape(-1)
    cone = rockets.project(rs, objects, camera, W, H, -1)
    for branch, name in enumerate(("the root where n > 0", "the root where n <= 0 and Aq < 0", "no root: Aq >= 0", "a root with d <= 0")):
        assert int((cone["branch"] == branch).sum()) >= BRANCH_MIN, f"{what}: {int((cone['branch'] == branch).sum())} records take '{name}'"
    h = groups["horizon"]
    assert not cone["visible"][h].any() and set(cone["branch"][h].tolist()) == {2, 3}, f"{what}: a rocket beyond the horizon shows"
    model = rockets.project(rs, objects, camera, W, H, interval)
    place = oracle_place(lib, view(camera, W, H, interval, 0), objects, rs)
    if interval == -1:
        assert not place["visible"][h].any(), f"{what}: the oracle shows a rocket beyond the horizon"
        assert np.array_equal(place["branch"][h], cone["branch"][h])
        for k in range(3):      # every class of acceleration is seen on both roots
            for branch in (0, 1):
                assert (place["visible"] & (place["branch"] == branch))[:groups["fast"].start][k::3].any(), f"{what}: {ACCELERATIONS[k]}, branch {branch}"
    t0, tb = pc.taps(place, rec, W, H, camera, 0.0), pc.taps(place, rec, W, H, camera, bias)
    assert (t0[:, 2] > 0).any(), f"{what}: no record in front of a hit pixel"
    assert (place["visible"] & (t0[:, 0] > t0[:, 1])).any(), f"{what}: no record hidden behind a hit pixel"
    assert (t0[:, 3] > 0).any(), f"{what}: no record over a miss pixel"
    assert (place["visible"] & (t0[:, 0] == 0)).any() or (camera.get("mode") == "equirect" and "h_fov" not in camera), f"{what}: no record outside the frame"
    assert (t0[groups["near"], 2] > 0).any() and (t0[groups["far"], 0] > t0[groups["far"], 1]).any()
    assert (tb[:, 1] >= t0[:, 1]).all()
    assert (t0[groups["fast"], 1] > 0).any(), f"{what}: no fast rocket is drawn"
    seen = int((t0[:, 1] > 0).sum())
    assert 0 < seen < len(rs), f"{what}: {seen} of {len(rs)} seen"
    assert int(model["visible"].sum()) > 0
    return place, t0, tb
