"""The rocket pass without a device: relativitypathtracer_amd.rockets.project, the float64 model, held to physics — the
ballistic model at acc = 0, a bisection on the sinh / cosh worldline, the Rindler horizon, the redshift seen from the pad, Bell's and
Born's fleets, and the convergence of inertial legs —; tests/native/rockets_oracle.c, the C restatement of the rules and the reference of
tests/test_gpu_rockets.py, held to the model; and the non-vacuity of tests/rockets_cases.py on CPU event frames.

The float32 bound (DESIGN.md §25 "How far float32 may put a record from the float64 model"; MEASURED on the crafted sets of this file,
times four — §24's convention —, not derived).  With eps = 2^-24, gamma = the rocket's Lorentz factor at emission in its object's frame
and A = the 2-norm of that object's InvLorentz, e = gamma A^2 eps:
    the camera directions differ by dn <= K_N e, which goes through §20's projection steps as its dn does;
    |d dist| / dist <= K_DIST e;   |d D| / D <= K_D e."""
import math

import numpy as np
import pytest

import ballistics_cases as bc
import events_oracle as eo
import particles_cases as pc
import rockets_cases as rc
import stars_cases as sc
from relativitypathtracer_amd import ballistics, rockets
from relativitypathtracer_amd.events import _objects_array
from test_ballistics_model import _position_ratios, identity_frame

EPS = 2.0 ** -24
# four times the largest figure measured on the 32 cases of test_the_c_oracle_puts_every_record_where_the_float64_model_does (K_N 784.9 —
# the smallest K inside the bound, found by bisection —, 744.21, 175.74): see DESIGN.md §25's table, and why the figures are what they
# are — a rocket that comes at the camera at gamma is 2 gamma^2 times nearer at the camera's time than when it sent its light, and the
# position at the camera's time is rounded at the scale of pos, not of that distance
K_N, K_DIST, K_D = 3140.0, 2977.0, 703.0


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return rc.build_library(tmp_path_factory.mktemp("rockets"))


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("rockets_events"))


_FRAMES = {}


def _frame(events_lib, scene_name, motion, interval, name, turned, W, H):
    """(scene, Object[] of the view, (H * W) records, camera) of tests/native/event_oracle.c, computed once per view."""
    key = (scene_name, motion, interval, name, turned, W, H)
    if key not in _FRAMES:
        scene = eo.load_scene(scene_name, motion, interval)
        cam = dict({k: v for k, v in rc.CAMERAS[name].items() if k != "orientation"}, orientation=sc.YPR if turned else None) if turned is not None else rc.CAMERAS[name]
        _FRAMES[key] = (scene, pc.scene_objects(scene, cam), sc.cpu_events(events_lib, scene, W, H, cam).reshape(-1), cam)
    return _FRAMES[key]


# ---- 1: acc = 0 is the ballistic model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", rc.INTERVALS)
@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("name", ["pinhole", "sphere"])
def test_without_acceleration_the_model_is_the_ballistic_model(events_lib, name, motion, interval):
    W, H = 128, 72
    scene, objects, records, camera = _frame(events_lib, "cubes", motion, interval, name, False, W, H)
    bs, groups, _ = bc.crafted(records, objects, camera, W, H, interval)
    for flags, inverse_square in ((0, False), (3, True)):
        want = ballistics.project(bs, objects, camera, W, H, interval, flags, dict(inverse_square=inverse_square))
        got = rockets.project(rockets.from_ballistics(bs), objects, camera, W, H, interval, flags, dict(inverse_square=inverse_square))
        assert np.array_equal(got["visible"], want["visible"]) and want["visible"].sum() > 500
        ok = want["visible"]
        for key in ("X", "Y", "dist", "D", "r", "te", "tau"):
            assert np.max(np.abs(got[key][ok] - want[key][ok]) / np.maximum(1.0, np.abs(want[key][ok]))) <= 1e-9, (key, flags)
        scale = np.maximum(np.abs(want["rgb"][ok]).max(axis=1, keepdims=True), 1e-300)
        assert np.max(np.abs(got["rgb"][ok] - want["rgb"][ok]) / scale) <= 1e-9, flags
        assert np.array_equal(got["z"][ok] < 0, want["tau"][ok] < 0) and np.max(np.abs(got["d"][ok] - 1.0)) == 0.0


# ---- 2: a bisection on the sinh / cosh worldline ------------------------------------------------------------------------------------
def _hyperbola(pos, u, acc, s):
    """X(s) = (0, pos) + U sinh(alpha s) / alpha + A (cosh(alpha s) - 1) / alpha^2, float64: (t (N,), x (N, 3))."""
    al = np.sqrt((acc * acc).sum(axis=1))
    g, a0, a = rockets.four_acceleration(u, acc)
    sh, ch1 = np.sinh(al * s) / al, (np.cosh(al * s) - 1.0) / (al * al)
    return g * sh + a0 * ch1, pos + u * sh[:, None] + a * ch1[:, None]


def _random_worldlines(n, seed):
    """n worldlines with a camera each: two thirds on the future light cone of an event of theirs at |alpha s| <= 10, one third moved
    beyond the horizon.  Returns (pos, u, acc, camera events (N, 4), s of the event or NaN)."""
    rng = np.random.default_rng(seed)
    pos = rng.normal(scale=5.0, size=(n, 3))
    u = rc._unit(rng, n) * rng.uniform(0.0, 3.0, n)[:, None]
    al = 10.0 ** rng.uniform(-2.0, 0.5, n)
    acc = rc._unit(rng, n) * al[:, None]
    s = rng.uniform(-10.0, 10.0, n) / al
    t, x = _hyperbola(pos, u, acc, s)
    way = 10.0 ** rng.uniform(-1.0, 2.0, n)
    cam = np.concatenate([(t + way)[:, None], x + way[:, None] * rc._unit(rng, n)], axis=1)
    beyond = np.arange(n) % 3 == 2
    # the horizon: the null plane (E - O).K = 0 through the hyperbola's centre O = (0, pos) - A / alpha^2, K = (A / alpha - U) / alpha;
    # seen iff (E - O).K > 0.  U.K = 1 / alpha: E - (h + margin) alpha U has (E - O).K = -margin
    g, a0, a = rockets.four_acceleration(u, acc)
    U, A = np.concatenate([g[:, None], u], axis=1), np.concatenate([a0[:, None], a], axis=1)
    O = np.concatenate([np.zeros((n, 1)), pos], axis=1) - A / (al * al)[:, None]
    K = (A / al[:, None] - U) / al[:, None]
    mink = lambda p, q: -p[:, 0] * q[:, 0] + (p[:, 1:] * q[:, 1:]).sum(axis=1)
    h = mink(cam - O, K)
    assert (h[~beyond] > 0).all()
    cam[beyond] = (cam - ((h + rng.uniform(0.01, 3.0, n) / al)[:, None] * al[:, None]) * U)[beyond]
    assert (mink(cam - O, K)[beyond] < 0).all()
    return pos, u, acc, cam, np.where(beyond, np.nan, s)


def _bisect(pos, u, acc, cam):
    """The emission event by bisection on F(s) = (T - t(s)) - |x(s) - C|, which falls with s: a root in alpha s in [-14, 14] iff
    F(-14 / alpha) > 0 (F at the upper end is below zero for every camera of _random_worldlines).  (seen, s, t, x)."""
    al = np.sqrt((acc * acc).sum(axis=1))

    def F(s):
        t, x = _hyperbola(pos, u, acc, s)
        return (cam[:, 0] - t) - np.linalg.norm(x - cam[:, 1:], axis=1)

    lo, hi = -14.0 / al, 14.0 / al
    seen = F(lo) > 0.0
    assert (F(hi) < 0.0).all()
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        up = F(mid) > 0.0
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    s = 0.5 * (lo + hi)
    t, x = _hyperbola(pos, u, acc, s)
    return seen, s, t, x


def test_the_closed_form_finds_the_event_a_bisection_finds():
    n = 3000
    pos, u, acc, cam, s_made = _random_worldlines(n, 25)
    seen, s, t, x = _bisect(pos, u, acc, cam)
    assert np.array_equal(seen, np.isfinite(s_made)) and 900 < (~seen).sum() < 1100
    frames = {"InvLorentz": np.broadcast_to(np.eye(4), (n, 4, 4)), "stationaryCam": cam}
    got = rockets.project_columns(pos, np.arange(n), np.ones((n, 3)), u, acc, np.full(n, -np.inf), np.full(n, np.inf), frames, dict(mode="equirect"), 128, 64, -1)
    assert np.array_equal(got["visible"], seen), "visibility differs"
    ok = seen
    scale = np.maximum(1.0, np.maximum(np.abs(t[ok]), np.linalg.norm(x[ok], axis=1)))
    err_t = np.abs(got["te"][ok] - t[ok]) / scale
    err_x = np.linalg.norm(got["pos_e"][ok] - x[ok], axis=1) / scale
    err_s = np.abs(got["s"][ok] - s[ok]) / np.maximum(1.0, np.abs(s[ok]))
    print(f"bisection: {ok.sum()} seen, {(~ok).sum()} beyond the horizon; largest relative error te {err_t.max():.2e}, pos {err_x.max():.2e}, s {err_s.max():.2e}")
    assert err_t.max() <= 1e-8 and err_x.max() <= 1e-8 and err_s.max() <= 1e-8
    assert np.max(np.abs(s[ok] - s_made[ok]) / np.maximum(1.0, np.abs(s[ok]))) <= 1e-8      # (the bisection finds the event the camera was put on)
    # r' is the camera's distance in the rocket's rest frame at emission: U(s).(X(s) - E)
    al = np.sqrt((acc * acc).sum(axis=1))
    g, a0, a = rockets.four_acceleration(u, acc)
    Ut = g * np.cosh(al * s) + a0 * np.sinh(al * s) / al
    Ux = u * np.cosh(al * s)[:, None] + a * (np.sinh(al * s) / al)[:, None]
    rest = -Ut * (t - cam[:, 0]) + (Ux * (x - cam[:, 1:])).sum(axis=1)
    mild = ok & (np.abs(al * s) <= 3.0)      # (beyond, the two terms of this reference cancel by more than the bisection's s allows)
    assert mild.sum() > 400 and np.max(np.abs(got["r"][mild] / rest[mild] - 1.0)) <= 1e-8


# ---- 3: the horizon ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.05, 1.0, 7.0])
def test_a_camera_sees_the_rocket_iff_it_is_above_the_null_plane(alpha):
    rng = np.random.default_rng(3)
    n = 600
    T = rng.uniform(-30.0, 30.0, n)
    C = rng.normal(scale=20.0, size=(n, 3))
    side = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    C[:, 0] = -T - 1.0 / alpha + side * 10.0 ** rng.uniform(-3.0, 1.5, n)       # T + C_x + 1 / alpha = +- (1e-3 .. 30), whatever C_y and C_z are
    height = T + C[:, 0] + 1.0 / alpha
    assert (np.abs(height) >= 0.99e-3).all() and (height > 0).sum() >= 200 and (height < 0).sum() >= 200
    frames = {"InvLorentz": np.broadcast_to(np.eye(4), (n, 4, 4)), "stationaryCam": np.concatenate([T[:, None], C], axis=1)}
    got = rockets.project_columns(np.zeros((n, 3)), np.arange(n), np.ones((n, 3)), np.zeros((n, 3)), np.tile((alpha, 0.0, 0.0), (n, 1)), np.full(n, -np.inf),
                                  np.full(n, np.inf), frames, dict(mode="equirect"), 128, 64, -1)
    assert np.array_equal(got["visible"], height > 0)
    assert set(got["branch"][height < 0].tolist()) <= {2, 3} and set(got["branch"][height > 0].tolist()) <= {0, 1}


# ---- 4: the redshift seen from the pad ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.01, 1.0, 30.0])
def test_from_the_pad_the_rocket_reddens_as_exp_minus_alpha_s(alpha):
    T = np.concatenate([[0.0], 10.0 ** np.linspace(-3.0, 3.0, 200)]) / alpha
    n = len(T)
    frames = {"InvLorentz": np.broadcast_to(np.eye(4), (n, 4, 4)), "stationaryCam": np.concatenate([T[:, None], np.zeros((n, 3))], axis=1)}
    origin = np.tile((0.0, 0.0, 1e-300), (n, 1))      # (a hair off the pad: at T = 0 the rocket IS the camera event, r' = 0)
    got = rockets.project_columns(origin, np.arange(n), np.ones((n, 3)), np.zeros((n, 3)), np.tile((0.0, 0.0, alpha), (n, 1)), np.full(n, -np.inf), np.full(n, np.inf),
                                  frames, dict(mode="equirect"), 128, 64, -1, 3)
    seen = got["visible"]
    assert seen[1:].all()
    want = rockets.redshift_from_pad(alpha, got["s"])
    assert np.max(np.abs(got["D"][seen] / want[seen] - 1.0)) <= 1e-12
    assert got["D"][seen].min() < 1e-3 and (np.diff(got["s"][1:]) > 0).all()
    # the light the pad sees at T left at the proper time s with exp(alpha s) = 1 + alpha T' ... the textbook: s = ln(1 + alpha T) / alpha
    assert np.max(np.abs(got["s"][1:] - np.log1p(alpha * T[1:]) / alpha) * alpha) <= 1e-12 * np.log1p(alpha * T[1:]).max() + 1e-13


# ---- 5: Bell's spaceships and a Born-rigid fleet on the slice ----------------------------------------------------------------------
def test_on_the_slice_a_bell_fleet_keeps_its_spacing_and_a_rigid_fleet_contracts():
    alpha, gap, n = 0.5, 1.0 / 64.0, 9          # (positions that are float32 numbers)
    x = np.stack([np.zeros(n), np.zeros(n), 10.0 + gap * np.arange(n)], axis=1)
    camera = dict(mode="equirect")
    for T in (0.0, 1.0, 4.0, 20.0):
        obj = identity_frame(T, (40.0, 0.0, 0.0))           # the camera at rest in the fleet's launch frame, off to the side
        bell = rockets.project(rockets.fleet(0, x, (0.0, 0.0, alpha)), obj, camera, 128, 64, 0)
        rigid = rockets.project(rockets.fleet(0, x, (0.0, 0.0, alpha), rigid=True), obj, camera, 128, 64, 0)
        assert bell["visible"].all() and rigid["visible"].all()
        assert np.max(np.abs(bell["te"] - T)) <= 1e-12 * max(1.0, T) and np.max(np.abs(rigid["te"] - T)) <= 1e-12 * max(1.0, T)
        # Bell: every rocket has moved by the same (sqrt(1 + (alpha T)^2) - 1) / alpha
        moved = (math.sqrt(1.0 + (alpha * T) ** 2) - 1.0) / alpha
        assert np.max(np.abs(bell["pos_e"][:, 2] - (x[:, 2] + moved))) <= 1e-12 * max(1.0, T)
        assert np.max(np.abs(np.diff(bell["pos_e"][:, 2]) / gap - 1.0)) <= 1e-9        # the spacing in the launch frame stays what it was
        # Born: rocket i sits at Rindler height X_i = 1 / alpha + (x_i - x_0) and is at sqrt(X_i^2 + T^2) from the common horizon's
        # vertex, so the gap to its neighbour is the launch gap over its OWN gamma = sqrt(1 + (T / X_i)^2), to first order in gap / X
        stored = rockets.fleet(0, x, (0.0, 0.0, alpha), rigid=True)
        X = 1.0 / np.linalg.norm(stored["acc"].astype(np.float64), axis=1)
        z0 = stored["pos"][:, 2].astype(np.float64)
        assert np.max(np.abs(rigid["pos_e"][:, 2] - (z0 - X + np.sqrt(X * X + T * T)))) <= 1e-9 * max(1.0, T)
        gamma = np.sqrt(1.0 + (T / X) ** 2)
        ratio = np.diff(rigid["pos_e"][:, 2]) / np.diff(z0)
        assert np.max(np.abs(ratio * gamma[:-1] - 1.0)) <= 2.0 * gap * alpha + 1e-5, (T, ratio * gamma[:-1])      # (float32 acc: X to 1e-7)
        if T >= 4.0:
            assert ratio.max() < 0.5


# ---- 6: inertial legs converge to the rocket ---------------------------------------------------------------------------------------
def test_ballistic_legs_approach_the_rocket_at_second_order():
    W, H = 1024, 512
    camera = dict(mode="equirect")
    one = rockets.from_arrays([(-3.0, 0.5, 6.0)], 0, (1.0, 1.0, 1.0), beta=(0.3, 0.0, 0.1), acc=(0.25, 0.1, -0.05), t0=0.0, t1=8.0)
    times = np.linspace(8.0, 14.0, 61)
    worst = {}
    for K in (16, 64):
        legs = rockets.as_ballistics(one, K)
        assert len(legs) == K and legs["t0"][0] == 0.0 and legs["t1"][-1] == 8.0 and np.array_equal(legs["t0"][1:], legs["t1"][:-1])
        worst[K], shown = 0.0, 0
        for T in times:
            obj = identity_frame(T)
            want = rockets.project(one, obj, camera, W, H, -1)
            got = ballistics.project(legs, obj, camera, W, H, -1)
            if not want["visible"][0]:
                continue
            # the leg whose window holds the rocket's emission time (at a joint a leg may miss its window by the error itself)
            k = min(K - 1, int((want["te"][0] - 0.0) / (8.0 / K)))
            free = legs[k:k + 1].copy()
            free["t0"], free["t1"] = -np.inf, np.inf
            leg = ballistics.project(free, obj, camera, W, H, -1)
            worst[K] = max(worst[K], math.hypot(leg["X"][0] - want["X"][0], leg["Y"][0] - want["Y"][0]))
            shown += int(got["visible"].sum() == 1)
        assert shown >= 0.9 * len(times)       # (nearly always exactly one leg shows)
    print(f"legs: largest screen error {worst[16]:.3e} px at K = 16, {worst[64]:.3e} px at K = 64, ratio {worst[16] / worst[64]:.2f}")
    assert worst[64] > 0.0 and worst[16] / worst[64] >= 4.0


# ---- the C oracle against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", rc.INTERVALS)
@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("turned", [False, True], ids=["straight", "turned"])
@pytest.mark.parametrize("name", ["pinhole", "lens", "sphere", "partial"])
def test_the_c_oracle_puts_every_record_where_the_float64_model_does(lib, events_lib, name, turned, motion, interval):
    W, H = 128, 72
    scene, objects, records, camera = _frame(events_lib, "cubes", motion, interval, name, turned, W, H)
    rs, groups, _ = rc.crafted(records, objects, camera, W, H, interval)
    rs = rs[np.r_[np.r_[groups["surface"], groups["near"], groups["far"], groups["on pixels"], groups["edges and corners"], groups["lattice"], groups["pile"]][:1200],
                  groups["fast"], groups["horizon"]]]
    got = rc.oracle_place(lib, rc.view(camera, W, H, interval, 3), objects, rs)
    want = rockets.project(rs, objects, camera, W, H, interval, 3)
    if interval == -1:
        assert np.array_equal(got["branch"], want["branch"]), np.nonzero(got["branch"] != want["branch"])[0][:10]
    A = np.linalg.norm(_objects_array(objects)["InvLorentz"].astype(np.float64), ord=2, axis=(1, 2))[rs["object"]]
    state = rockets.advance(rs["pos"].astype(np.float64), rs["u"].astype(np.float64), rs["acc"].astype(np.float64), np.where(np.isfinite(want["te"]), want["te"], 0.0))
    gamma = np.sqrt(1.0 + (state[1] ** 2).sum(axis=1))
    e = gamma * A * A * EPS
    rx, ry, both = _position_ratios(got, want, camera, W, H, K_N * e)
    assert both.sum() >= 100, both.sum()
    lo, hi = 1e-3, 1e6           # the smallest K with |dX| and |dY| inside the bound (the bound is not linear in K: bisect)
    for _ in range(50):
        mid = math.sqrt(lo * hi)
        qx, qy, _ = _position_ratios(got, want, camera, W, H, mid * e)
        lo, hi = (lo, mid) if max(qx[both].max(), qy[both].max()) <= 1.0 else (mid, hi)
    rel_dist = np.abs(got["dist"][both] / want["dist"][both] - 1.0) / e[both]
    line = f"{name} turned={turned} {motion} interval={interval}: {both.sum()} records, smallest K_N {hi:.3f}, " \
           f"|d dist| / (dist e) {rel_dist.max():.3f}"
    if interval == -1:
        rel_D = np.abs(got["D"][both] / want["D"][both] - 1.0) / e[both]
        line += f", |d D| / (D e) {rel_D.max():.3f}"
    print(line)
    assert rx[both].max() <= 1.0 and ry[both].max() <= 1.0, line
    assert rel_dist.max() <= K_DIST, line
    if interval == -1:
        assert rel_D.max() <= K_D, line
    for flags in rc.FLAGS:
        for inverse_square in (False, True):
            g = rc.oracle_place(lib, rc.view(camera, W, H, interval, flags, inverse_square=inverse_square), objects, rs)
            w = rockets.project(rs, objects, camera, W, H, interval, flags, dict(inverse_square=inverse_square))
            ok = g["visible"] & w["visible"]
            amp = np.maximum(1.0, w["D"][ok] ** 2) / (w["r"][ok] ** 2 if inverse_square else 1.0)
            scale = (rs["rgb"][ok].astype(np.float64).max(axis=1) * amp)[:, None]
            assert np.max(np.abs(g["rgb"][ok] - w["rgb"][ok]) / scale) <= max(1e-4, 10.0 * K_D * e[ok].max()), (flags, inverse_square)


# ---- the front end ------------------------------------------------------------------------------------------------------------------
def test_from_arrays_launch_fleet_trip_save_and_load(tmp_path):
    one = rockets.from_arrays([(1.0, 2.0, 3.0)], 2, (0.5, 0.25, 1.0), beta=(0.6, 0.0, 0.0), acc=(0.0, 0.5, 0.0), t0=1.0, t1=4.0)
    assert one["object"][0] == 2 and one["u"][0].tolist() == [0.75, 0.0, 0.0] and one["pos"][0].tolist() == [1.0, 2.0, 3.0] and one["acc"][0].tolist() == [0.0, 0.5, 0.0]
    assert one["t0"][0] == 1.0 and one["t1"][0] == 4.0 and one["reserved"][0] == 0.0
    # an epoch is moved along the hyperbola: the worldline through (10, pos) is the worldline through where it was at time 0
    moved = rockets.from_arrays([(1.0, 2.0, 3.0)], 2, (0.5, 0.25, 1.0), beta=(0.6, 0.0, 0.0), acc=(0.0, 0.5, 0.0), epoch=10.0)
    back = rockets.advance(moved["pos"].astype(np.float64), moved["u"].astype(np.float64), moved["acc"].astype(np.float64), 10.0)
    assert np.allclose(back[0], [(1.0, 2.0, 3.0)], atol=1e-5) and np.allclose(back[1], [(0.75, 0.0, 0.0)], atol=1e-6) and np.allclose(back[2], [(0.0, 0.5, 0.0)], atol=1e-6)
    assert abs(np.linalg.norm(moved["acc"][0]) - 0.5) < 1e-6
    with pytest.raises(ValueError):
        rockets.from_arrays([(0.0, 0.0, 0.0)], 0, (1.0, 1.0, 1.0), beta=(0.1, 0.0, 0.0), u=(0.1, 0.0, 0.0))
    still = rockets.from_ballistics(ballistics.jet(1, (0.0, 0.0, 5.0), (0.0, 0.0, -2.0), 0.8, [0.0, 1.0, 2.0], (1.0, 0.0, 0.0)))
    assert len(still) == 3 and not still["acc"].any() and still["t0"].tolist() == [0.0, 1.0, 2.0] and (still["object"] == 1).all()
    up = rockets.launch(0, (0.0, 0.0, 5.0), (0.0, 0.0, 1.0), [0.0, 2.0], (1.0, 1.0, 1.0))
    assert up["t0"].tolist() == [0.0, 2.0] and up["pos"][0].tolist() == [0.0, 0.0, 5.0]
    at_two = rockets.advance(up["pos"][1:].astype(np.float64), up["u"][1:].astype(np.float64), up["acc"][1:].astype(np.float64), 2.0)
    assert np.allclose(at_two[0], [(0.0, 0.0, 5.0)], atol=1e-5) and np.allclose(at_two[1], 0.0, atol=1e-6)      # at rest on the pad when it leaves
    assert len(rockets.launch(0, (0.0, 0.0, 5.0), (0.0, 0.0, 1.0), 3, (1.0, 1.0, 1.0))) == 3
    x = np.stack([np.zeros(3), np.zeros(3), [0.0, 1.0, 3.0]], axis=1)
    assert np.allclose(np.linalg.norm(rockets.fleet(0, x, (0.0, 0.0, 0.5))["acc"], axis=1), 0.5)
    assert np.allclose(np.linalg.norm(rockets.fleet(0, x, (0.0, 0.0, 0.5), rigid=True)["acc"], axis=1), [0.5, 1.0 / 3.0, 0.2])
    with pytest.raises(ValueError):
        rockets.fleet(0, x[::-1], (0.0, 0.0, 0.5), rigid=True)          # the last rocket would lie behind the horizon
    legs = rockets.trip(0, (1.0, 0.0, 0.0), (0.0, 0.0, 2.0), 1.0, 1.5, (1.0, 1.0, 1.0))
    assert len(legs) == 4 and legs["t0"][0] == 0.0 and np.array_equal(legs["t0"][1:], legs["t1"][:-1])
    assert np.allclose(legs["t1"], np.arange(1, 5) * math.sinh(1.5), rtol=1e-6)
    ends = [rockets.advance(legs["pos"][k:k + 1].astype(np.float64), legs["u"][k:k + 1].astype(np.float64), legs["acc"][k:k + 1].astype(np.float64),
                            float(legs["t1"][k])) for k in range(4)]
    far = math.cosh(1.5) - 1.0
    assert np.allclose([e[0][0, 2] for e in ends], [far, 2 * far, far, 0.0], atol=1e-4) and np.allclose(ends[3][1], 0.0, atol=1e-5)
    assert abs(ends[0][3][0] - 1.5) < 1e-6                   # the first leg's proper time
    path = tmp_path / "set.bin"
    rockets.save(path, legs)
    assert path.stat().st_size == 64 * 4 and rockets.load(path).tobytes() == legs.tobytes()
    path.write_bytes(b"\0" * 65)
    with pytest.raises(ValueError):
        rockets.load(path)
    with pytest.raises(ValueError):
        rockets.project(legs, identity_frame(), dict(mode="pinhole"), 64, 32, 2)
    with pytest.raises(ValueError):
        rockets.as_ballistics(up, 4)            # an open window has no K equal parts
    assert rockets.redshift_from_pad(2.0, 0.5) == pytest.approx(math.exp(-1.0))


# ---- the non-vacuity of the GPU cases, on CPU event frames ------------------------------------------------------------------------
@pytest.mark.parametrize("size", rc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(rc.CAMERAS))
@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("scene_name", rc.SCENES)
def test_the_shared_cases_show_something(lib, events_lib, scene_name, motion, name, size):
    W, H = size
    camera = rc.CAMERAS[name]
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    pixels["rgba"] = (40, 50, 60, 1)
    for interval in rc.INTERVALS:
        what = f"{scene_name} {motion} {name} {W}x{H} interval {interval}"
        scene, objects, records, _ = _frame(events_lib, scene_name, motion, interval, name, None, W, H)
        rs, groups, bias = rc.crafted(records, objects, camera, W, H, interval)
        place, t0, tb = rc.check_shows_something(lib, records, objects, camera, W, H, interval, rs, groups, bias, what)
        for flags in rc.FLAGS:
            after, (seen, changed) = rc.oracle_pass(lib, rc.view(camera, W, H, interval, flags), objects, rs, pixels, records)
            assert 0 < seen < len(rs) and changed > 0, what
            assert seen == int((t0[:, 1] > 0).sum()), f"{what}: the oracle saw {seen} records, the taps in numpy {int((t0[:, 1] > 0).sum())}"
            assert (after["rgba"][:, 3] == 1).all() and np.array_equal(after["x"], pixels["x"]) and np.array_equal(after["unspecified"], pixels["unspecified"])
        biased, (seen_biased, _) = rc.oracle_pass(lib, rc.view(camera, W, H, interval, 0, depth_bias=bias), objects, rs, pixels, records)
        assert seen_biased == int((tb[:, 1] > 0).sum()) >= seen
