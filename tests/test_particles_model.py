"""The particle pass without a device: the round trip through the renderer's own records — a particle placed on a hit
pixel's recorded event projects back onto that pixel, at the record's dist —; tests/native/particles_oracle.c, the C restatement of the
rules and the reference of tests/test_gpu_particles.py, against relativitypathtracer_amd.particles.project, the float64 model; the model
against special relativity; and the non-vacuity of tests/particles_cases.py on CPU event frames.

The position bound (DESIGN.md §20 "How far float32 may put a particle from the float64 model"; DERIVED, not measured) with eps = 2^-24
and a = the 2-norm of the particle's object's InvLorentz (gamma (1 + beta) of the object's motion in the camera frame), per particle:
    dn  = (16.5 a^2 + 4) eps                             the angle between the two camera directions
    |d dist| / dist <= (16.5 a^2 + 2.5) eps
and then §19's projection steps with this dn:
    pinhole:   |dX| <= 1.01 W / (2 s aspect) (1 / n.z + |n.x| / n.z^2) dn + 5 eps (|X| + W), Y likewise with H / (2 s) and n.y
    equirect:  |dX| <= (W / h_fov) (min(1.01 dn / h, 2 pi) + 100 eps) + 4 eps (|X| + W), h = hypot(n.x, n.z), X compared modulo a turn;
               |dY| <= (H / v_fov) (min(1.01 dn / h, 1.01 sqrt(2 dn)) + 20 eps) + 4 eps (|Y| + H)"""
import math

import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
from relativitypathtracer_amd import particles
from relativitypathtracer_amd.events import _objects_array
from relativitypathtracer_amd.scene import OBJECT_DTYPE

EPS = 2.0 ** -24
ROUND_TRIP_CAMERAS = {"pinhole": dict(mode="pinhole"), "lens": dict(mode="pinhole", v_fov=math.radians(60.0)), "equirect": dict(mode="equirect")}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return pc.build_library(tmp_path_factory.mktemp("particles"))


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("particles_events"))


_FRAMES = {}


def _frame(events_lib, scene_name, motion, interval, camera_name, camera, turned, W, H):
    """(scene, Object[] of the view, (H * W) records) of tests/native/event_oracle.c, computed once per view."""
    key = (scene_name, motion, interval, camera_name, turned, W, H)
    if key not in _FRAMES:
        scene = eo.load_scene(scene_name, motion, interval)
        cam = dict(camera, orientation=sc.YPR if turned else None)
        _FRAMES[key] = (scene, pc.scene_objects(scene, cam), sc.cpu_events(events_lib, scene, W, H, cam).reshape(-1), cam)
    return _FRAMES[key]


# ---- the round trip through the renderer's own records --------------------------------------------------------------------------
# Views with fewer than 40 hit pixels are no case (4 to 38 of them): at 0.9c with light delay the scenes shrink ahead of the camera, so
# the 67 x 41 pinhole and the panorama (whose pixels are larger still) see too little — all but `arch` in the 128 x 72 panorama, not turned
def _too_few_hits(scene_name, size, camera_name, turned, motion, interval):
    if motion != "0.9c" or interval != -1:
        return False
    if camera_name == "pinhole":
        return size == (67, 41)
    if camera_name == "equirect":
        return not (scene_name == "arch" and size == (128, 72) and not turned)
    return False


ROUND_TRIPS = [(s, z, c, t, m, i) for s in ("cubes", "arch", "rulers") for z in ((128, 72), (67, 41)) for c in ROUND_TRIP_CAMERAS
               for t in (False, True) for m in ("rest", "0.9c") for i in (-1, 0) if not _too_few_hits(s, z, c, t, m, i)]


@pytest.mark.parametrize("scene_name,size,camera_name,turned,motion,interval", ROUND_TRIPS,
                         ids=[f"{s}-{z[0]}x{z[1]}-{c}-{'turned' if t else 'straight'}-{m}-{i}" for s, z, c, t, m, i in ROUND_TRIPS])
def test_a_particle_on_a_recorded_event_comes_back_to_its_pixel(events_lib, scene_name, size, camera_name, turned, motion, interval):
    """2e-3 px and 4e-5 relative: about four times the 4.6e-4 px and 8.2e-6 measured for the pinhole at 128 x 72 (the residual is the
    float32 rounding of the recorded event).  Every hit pixel of every view."""
    W, H = size
    scene, objects, records, camera = _frame(events_lib, scene_name, motion, interval, camera_name, ROUND_TRIP_CAMERAS[camera_name], turned, W, H)
    hit = np.nonzero(records["object"] >= 0)[0]
    assert len(hit) >= 40, f"{len(hit)} hit pixels"
    ps = particles.at_events(records, (1.0, 1.0, 1.0))
    assert len(ps) == len(hit)
    p = particles.project(ps, objects, camera, W, H, interval)
    assert p["visible"].all(), f"{int((~p['visible']).sum())} of {len(hit)} particles are not visible"
    dx, dy = p["X"] - (hit % W), p["Y"] - (hit // W)
    if camera["mode"] == "equirect":
        dx = (dx + W / 2) % W - W / 2
    rel = np.abs(p["dist"] / records["dist"][hit].astype(np.float64) - 1.0)
    print(f"{len(hit)} hit pixels: largest |dX| {np.abs(dx).max():.3g} px, |dY| {np.abs(dy).max():.3g} px, |dist / record - 1| {rel.max():.3g}")
    assert np.abs(dx).max() <= 2e-3 and np.abs(dy).max() <= 2e-3
    assert rel.max() <= 4e-5
    if interval == -1:      # the emission time is the record's
        te = np.abs(p["te"] - records["event"][hit, 0].astype(np.float64))
        assert te.max() <= 1e-3 * max(1.0, float(np.abs(records["event"][hit, 0]).max()))


# ---- the C oracle against the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", pc.INTERVALS)
@pytest.mark.parametrize("motion", pc.MOTIONS)
@pytest.mark.parametrize("turned", [False, True], ids=["straight", "turned"])
@pytest.mark.parametrize("name", ["pinhole", "lens", "sphere", "partial"])
def test_the_c_oracle_puts_every_particle_where_the_float64_model_does(lib, events_lib, name, turned, motion, interval):
    W, H = 128, 72
    scene, objects, records, camera = _frame(events_lib, "cubes", motion, interval, "oracle " + name, {k: v for k, v in pc.CAMERAS[name].items() if k != "orientation"}, turned, W, H)
    ps, groups, _ = pc.crafted(records, objects, camera, W, H, interval)
    ps = ps[np.r_[groups["surface"], groups["near"], groups["far"], groups["on pixels"], groups["edges and corners"], groups["lattice"]]]
    got = pc.oracle_place(lib, pc.view(camera, W, H, interval, 0), objects, ps)
    want = particles.project(ps, objects, camera, W, H, interval)
    a = np.linalg.norm(_objects_array(objects)["InvLorentz"].astype(np.float64), ord=2, axis=(1, 2))[ps["object"]]
    dn = (16.5 * a * a + 4.0) * EPS
    n = want["n"]
    both = got["visible"] & want["visible"]
    if camera["mode"] == "pinhole":
        s = float(eo.lens_scale(camera["v_fov"])) if camera.get("v_fov") else 1.0
        both &= n[:, 2] >= 0.05
        with np.errstate(all="ignore"):
            tol_x = 1.01 * W / (2 * s * (W / H)) * (1 / n[:, 2] + np.abs(n[:, 0]) / n[:, 2] ** 2) * dn + 5 * EPS * (np.abs(want["X"]) + W)
            tol_y = 1.01 * H / (2 * s) * (1 / n[:, 2] + np.abs(n[:, 1]) / n[:, 2] ** 2) * dn + 5 * EPS * (np.abs(want["Y"]) + H)
        dx = got["X"] - want["X"]
    else:
        assert got["visible"].all() and want["visible"].all()
        h_fov, v_fov = float(np.float32(camera.get("h_fov", 2 * math.pi))), float(np.float32(camera.get("v_fov", math.pi)))
        h = np.hypot(n[:, 0], n[:, 2])
        with np.errstate(all="ignore"):
            tol_x = W / h_fov * (np.minimum(1.01 * dn / h, 2 * math.pi) + 100 * EPS) + 4 * EPS * (np.abs(want["X"]) + W)
            tol_y = H / v_fov * (np.minimum(1.01 * dn / h, 1.01 * math.sqrt(2 * dn.max())) + 20 * EPS) + 4 * EPS * (np.abs(want["Y"]) + H)
        turn = W * 2 * math.pi / h_fov
        dx = (got["X"] - want["X"] + turn / 2) % turn - turn / 2
    dy = got["Y"] - want["Y"]
    assert both.sum() >= 100, both.sum()
    worst_x, worst_y = np.max(np.abs(dx[both]) / tol_x[both]), np.max(np.abs(dy[both]) / tol_y[both])
    rel = np.abs(got["dist"][both] / want["dist"][both] - 1.0) / ((16.5 * a[both] ** 2 + 2.5) * EPS)
    print(f"{name} turned={turned} {motion} interval={interval}: {both.sum()} particles, largest |dX| / bound {worst_x:.3f}, |dY| / bound {worst_y:.3f}, "
          f"|d dist| / bound {rel.max():.3f}, largest |dX| {np.max(np.abs(dx[both])):.3g} px, largest a {a.max():.3f}")
    assert worst_x <= 1.0 and worst_y <= 1.0 and rel.max() <= 1.0
    # the bound itself is below half a pixel inside the frame (but at the panorama's poles, where the longitude means nothing: two of
    # the crafted particles sit there)
    off_pole = np.hypot(n[:, 0], n[:, 2]) > 1e-3
    assert np.max(tol_x[both & off_pole & (np.abs(want["X"] - W / 2) < W / 2)]) < 0.5
    # the colours: rule 3 in float32 against float64, every Doppler setting, with and without the inverse square
    for flags in pc.FLAGS:
        for inverse_square in (False, True):
            g = pc.oracle_place(lib, pc.view(camera, W, H, interval, flags, inverse_square=inverse_square), objects, ps)
            w = particles.project(ps, objects, camera, W, H, interval, flags, dict(inverse_square=inverse_square))
            ok = g["visible"] & w["visible"]
            # against the particle's own scale: its rest colour times what rule 3 can multiply it by (near the band's edges the
            # shifted colour itself goes to zero).  The spectrum's slope is at most 1 / (nu_R - K0) = 4.6 per unit of nu, so 1e-4
            # covers D's rounding at a = 4.4 many times over
            amp = np.maximum(1.0, w["D"][ok] ** 2) / (w["r"][ok] ** 2 if inverse_square else 1.0)
            scale = (ps["rgb"][ok].astype(np.float64).max(axis=1) * amp)[:, None]
            assert np.max(np.abs(g["rgb"][ok] - w["rgb"][ok]) / scale) <= 1e-4, (flags, inverse_square)


# ---- the model against special relativity ---------------------------------------------------------------------------------------
GAMMAS = {3.0 / 5.0: 5.0 / 4.0, 15.0 / 17.0: 17.0 / 8.0, 63.0 / 65.0: 65.0 / 16.0}      # Pythagorean triples: gamma and gamma beta are floats


def boosted_object(beta, cam=(0.0, 0.0, 0.0, 0.0)):
    """One Object whose rest frame moves at beta along +z through the camera's: InvLorentz = the boost rest -> camera."""
    g = GAMMAS[abs(beta)]
    o = np.zeros(1, dtype=OBJECT_DTYPE)
    o["InvLorentz"][0] = [[g, 0, 0, g * beta], [0, 1, 0, 0], [0, 0, 1, 0], [g * beta, 0, 0, g]]
    o["Lorentz"][0] = [[g, 0, 0, -g * beta], [0, 1, 0, 0], [0, 0, 1, 0], [-g * beta, 0, 0, g]]
    o["stationaryCam"][0] = cam
    assert float(o["InvLorentz"][0, 0, 0]) == g and float(o["InvLorentz"][0, 0, 3]) == g * beta and abs(g * g * (1.0 - beta * beta) - 1.0) < 1e-15
    return o


CAMERA = dict(mode="equirect")


@pytest.mark.parametrize("beta", [3.0 / 5.0, 15.0 / 17.0, 63.0 / 65.0, -3.0 / 5.0, -15.0 / 17.0, -63.0 / 65.0])
def test_a_particle_on_the_line_of_sight_has_the_longitudinal_doppler_factor(beta):
    """Ahead of the camera (+z) in a frame that moves at beta along +z: receding for beta > 0, D = sqrt((1 - beta) / (1 + beta))."""
    ps = particles.from_arrays([(0.0, 0.0, 2.0), (0.0, 0.0, 0.5), (0.0, 0.0, 64.0)], 0, (1.0, 0.5, 0.25))
    p = particles.project(ps, boosted_object(beta), CAMERA, 64, 32, -1)
    assert p["visible"].all()
    assert np.max(np.abs(p["D"] / math.sqrt((1.0 - beta) / (1.0 + beta)) - 1.0)) <= 1e-12
    assert np.max(np.abs(p["n"] - (0.0, 0.0, 1.0))) <= 1e-12
    # ... and behind the camera the same frame approaches
    behind = particles.project(particles.from_arrays([(0.0, 0.0, -2.0)], 0, (1.0, 1.0, 1.0)), boosted_object(beta), CAMERA, 64, 32, -1)
    assert abs(behind["D"][0] / math.sqrt((1.0 + beta) / (1.0 - beta)) - 1.0) <= 1e-12


@pytest.mark.parametrize("beta", [3.0 / 5.0, -15.0 / 17.0])
def test_the_bolometric_flux_is_the_textbook_law(beta):
    """Inverse square and bolometric beaming: rgb D^2 / r^2 == rgb D^4 / dist^2."""
    rng = np.random.default_rng(7)
    ps = particles.from_arrays(rng.uniform(-6.0, 6.0, (500, 3)), 0, rng.uniform(0.1, 2.0, (500, 3)))
    obj = boosted_object(beta, (0.25, 0.5, -0.75, 1.5))
    p = particles.project(ps, obj, CAMERA, 64, 32, -1, 2, dict(inverse_square=True))
    assert p["visible"].all() and p["D"].min() < 0.8 and p["D"].max() > 1.2
    want = ps["rgb"].astype(np.float64) * (p["D"] ** 4 / p["dist"] ** 2)[:, None]
    assert np.max(np.abs(p["rgb"] / want - 1.0)) <= 1e-12
    # the null vector: |k.yzw| = -k.x
    assert np.max(np.abs(p["dist"] / -p["k"][:, 0] - 1.0)) <= 1e-12
    # without beaming the inverse square alone; without either, the colour as given
    alone = particles.project(ps, obj, CAMERA, 64, 32, -1, 0, dict(inverse_square=True))
    assert np.max(np.abs(alone["rgb"] / (ps["rgb"].astype(np.float64) / (p["r"] ** 2)[:, None]) - 1.0)) <= 1e-12
    assert np.array_equal(particles.project(ps, obj, CAMERA, 64, 32, -1)["rgb"], ps["rgb"].astype(np.float64))


@pytest.mark.parametrize("beta", [3.0 / 5.0, -63.0 / 65.0])
def test_with_light_delay_off_the_particle_is_seen_on_the_cameras_simultaneity_slice(beta):
    rng = np.random.default_rng(8)
    ps = particles.from_arrays(rng.uniform(-6.0, 6.0, (500, 3)), 0, (1.0, 1.0, 1.0))
    p = particles.project(ps, boosted_object(beta, (0.25, 0.5, -0.75, 1.5)), CAMERA, 64, 32, 0, 3)
    assert p["visible"].all()
    assert np.max(np.abs(p["k"][:, 0]) / p["r"]) <= 1e-12
    assert np.all(p["D"] == 1.0) and np.array_equal(p["rgb"], ps["rgb"].astype(np.float64))      # Doppler is off with the light delay


def test_a_particle_outside_its_objects_window_is_skipped():
    obj = boosted_object(3.0 / 5.0, (10.0, 0.0, 0.0, 0.0))
    ps = particles.from_arrays([(0.0, 0.0, 2.0), (0.0, 3.0, 4.0), (0.0, 0.0, 8.0)], 0, (1.0, 1.0, 1.0))       # r = 2, 5, 8: te = 8, 5, 2
    free = particles.project(ps, obj, CAMERA, 64, 32, -1)
    assert free["visible"].all() and free["te"].tolist() == [8.0, 5.0, 2.0]
    for window, want in (((-math.inf, math.inf), [True, True, True]), ((4.0, 6.0), [False, True, False]), ((5.0, 8.0), [False, True, False]),
                         ((2.0, 5.0), [False, False, True]), ((8.0, math.inf), [True, False, False]), ((6.0, 6.0), [False, False, False]),
                         ((-math.inf, 2.0), [False, False, False])):
        got = particles.project(ps, obj, CAMERA, 64, 32, -1, windows=[window])
        assert got["visible"].tolist() == want, window        # in(W, t): t0 <= t < t1
        assert np.isnan(got["X"][~got["visible"]]).all()


def test_lattice_at_events_save_and_load(tmp_path):
    grid = particles.lattice(3, (-1.0, 0.0, 2.0), (1.0, 0.5, 2.0), (3, 2, 1), (0.5, 0.25, 1.0))
    assert len(grid) == 6 and (grid["object"] == 3).all() and grid["pos"][:3, 0].tolist() == [-1.0, 0.0, 1.0] and grid["pos"][3, 1] == 0.5
    assert len(particles.lattice(0, (0, 0, 0), (1, 1, 1), 4, (1, 1, 1))) == 64
    records = np.zeros((2, 3), dtype=eo.EVENT_DTYPE)
    records["object"] = [[-1, 2, 2], [5, -1, 0]]
    records["event"][..., 1:] = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    ps = particles.at_events(records, (1.0, 0.0, 0.0))
    assert ps["object"].tolist() == [2, 2, 5, 0] and ps["pos"][0].tolist() == [3.0, 4.0, 5.0] and ps["pos"][3].tolist() == [15.0, 16.0, 17.0]
    assert particles.at_events(records, (1.0, 0.0, 0.0), stride=2)["object"].tolist() == [2, 5]
    path = tmp_path / "set.bin"
    particles.save(path, ps)
    assert path.stat().st_size == 32 * 4 and particles.load(path).tobytes() == ps.tobytes()
    path.write_bytes(b"\0" * 33)
    with pytest.raises(ValueError):
        particles.load(path)
    with pytest.raises(ValueError):
        particles.project(ps, boosted_object(0.6), CAMERA, 64, 32, 2)


# ---- the non-vacuity of the GPU cases, on CPU event frames ------------------------------------------------------------------------
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(pc.CAMERAS))
@pytest.mark.parametrize("motion", pc.MOTIONS)
@pytest.mark.parametrize("scene_name", pc.SCENES)
def test_the_shared_cases_show_something(lib, events_lib, scene_name, motion, name, size):
    W, H = size
    camera = pc.CAMERAS[name]
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    pixels["rgba"] = (40, 50, 60, 1)
    for interval in pc.INTERVALS:
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        scene = eo.load_scene(scene_name, motion, interval)
        objects = pc.scene_objects(scene, camera)
        records = sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1)
        ps, groups, bias = pc.crafted(records, objects, camera, W, H, interval)
        place, t0, tb = pc.check_shows_something(lib, records, objects, camera, W, H, interval, ps, groups, bias, what)
        hit = records["object"] >= 0
        for flags in pc.FLAGS:
            after, (seen, changed) = pc.oracle_pass(lib, pc.view(camera, W, H, interval, flags), objects, ps, pixels, records)
            assert 0 < seen < len(ps) and changed > 0, what
            assert seen == int((t0[:, 1] > 0).sum()), f"{what}: the oracle saw {seen} particles, the taps in numpy {int((t0[:, 1] > 0).sum())}"
            diff = (after["rgba"] != pixels["rgba"]).any(axis=1)
            if not flags & 1:       # (at 0.9c the shift moves the crafted colours out of the band)
                assert diff[hit].any() and diff[~hit].any(), f"{what}: particles show over hit pixels and over miss pixels"
            assert (after["rgba"][:, 3] == 1).all() and np.array_equal(after["x"], pixels["x"]) and np.array_equal(after["unspecified"], pixels["unspecified"])
            if not flags & 1:
                k = int(np.floor(place["Y"][groups["pile"]][0])) * W + int(np.floor(place["X"][groups["pile"]][0]))
                assert after["rgba"][k, 0] == 255 and after["rgba"][k, 1] == 255, "1000 particles on one pixel saturate it"
        biased, (seen_biased, _) = pc.oracle_pass(lib, pc.view(camera, W, H, interval, 0, depth_bias=bias), objects, ps, pixels, records)
        assert seen_biased == int((tb[:, 1] > 0).sum()) >= seen


def test_the_windowed_case_shows_one_leg(lib, events_lib):
    W, H = 128, 72
    wl, scene, ps = pc.turnaround()
    camera = pc.CAMERAS["pinhole"]
    windows = scene.windows()
    assert windows is not None and len(wl) == 3 and np.array_equal(windows[:3], wl.windows())
    objects = pc.scene_objects(scene, camera)
    free = pc.oracle_place(lib, pc.view(camera, W, H, -1, 0), objects, ps)
    held = pc.oracle_place(lib, pc.view(camera, W, H, -1, 0), objects, ps, windows)
    legs = [ps["object"] == j for j in range(3)]
    in_frame = free["visible"] & (free["X"] > 0) & (free["X"] < W - 1) & (free["Y"] > 0) & (free["Y"] < H - 1)
    assert sum(in_frame[m].any() for m in legs) >= 2, "without the windows the lamps of two legs at least are in the frame at once"
    shown = [bool(held["visible"][m].any()) for m in legs]
    assert sum(shown) >= 1 and not all(shown), f"legs whose lamps show: {shown}"
    assert (free["visible"] & ~held["visible"]).any(), "no particle is windowed out"
    for j, m in enumerate(legs):        # a leg shows exactly the lamps whose emission time its window holds
        t0, t1 = windows[j]
        assert np.array_equal(held["visible"][m], free["visible"][m] & ~(free["te"][m] < t0) & ~(free["te"][m] >= t1))
    # with every window at its default the pass is the un-windowed one
    records = sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1)
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    default = np.tile(np.array([-np.inf, np.inf], dtype=np.float32), (len(windows), 1))
    v = pc.view(camera, W, H, -1, 3)
    plain = pc.oracle_pass(lib, v, objects, ps, pixels, records)
    assert pc.oracle_pass(lib, v, objects, ps, pixels, records, default)[0].tobytes() == plain[0].tobytes()
    windowed = pc.oracle_pass(lib, v, objects, ps, pixels, records, windows)
    assert 0 < windowed[1][0] < plain[1][0]
