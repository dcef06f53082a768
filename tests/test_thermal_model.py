"""The thermal point sources without a device: tests/native/thermal_oracle.c — the C restatement of T_f and of both
passes with it, the reference of tests/test_gpu_thermal_*.py — against relativitypathtracer_amd.stars.thermal_colour, the float64 model;
the numpy float32 restatement against the C one, bit for bit; the model's identities; the test that shows the feature (stars ahead of a
camera at gamma = 5 that S_f blacks out and the thermal law colours as blackbodies of D T); and the non-vacuity of tests/thermal_cases.py.

The error bound (DESIGN.md §21 "Error"), per channel, with u = 2^-24, x = x_k and y = x / D:
    |T_f32 - T_f| <= (3 x + 4 y + |x - y| + 30) u |T_f|      wherever x - y >= -85 (below that the float32 operator returns 0 from -86 on)
Largest error seen over the inputs of test_the_c_operator_stays_inside_the_derived_bound: 0.56 of the bound with the shift alone, 0.63
with shift and beaming (printed by the test); the bound itself is 5.5e-5 at its largest (x = 66, D = 1e-3 .. 1e3 with x - y >= -85)."""
import math

import numpy as np
import pytest

import events_oracle as eo
import particles_cases as pc
import stars_cases as sc
import thermal_cases as tc
from relativitypathtracer_amd import particles, stars


@pytest.fixture(scope="module")
def stars_lib(tmp_path_factory):
    return tc.build_stars_library(tmp_path_factory.mktemp("thermal_stars"))


@pytest.fixture(scope="module")
def particles_lib(tmp_path_factory):
    return tc.build_particles_library(tmp_path_factory.mktemp("thermal_particles"))


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("thermal_events"))


def S(flags, D, rgb):
    """S_f in float64 (stars.point_source_colour without its / D^2)."""
    o = stars.point_source_colour(flags, D, rgb)
    return o * (np.asarray(D, dtype=np.float64) ** 2)[:, None] if flags & 2 else o


def planck(T):
    """Un-normalised Planck samples nu_k^3 / expm1(x_k) at the three primaries, (n, 3) float64."""
    T = np.asarray(T, dtype=np.float64)[:, None]
    lam = np.asarray(stars.WAVELENGTHS_NM)
    return (1.0 / lam) ** 3 / np.expm1(stars._HC_OVER_K_NM / (lam * T))


# ---- the C operator against the float64 model ---------------------------------------------------------------------------------------
def test_the_host_conversion_is_pythons_double_rounded_once(stars_lib):
    T = np.concatenate([[0.0, tc.T_MIN, tc.T_MAX], np.exp(np.random.default_rng(1).uniform(math.log(tc.T_MIN), math.log(tc.T_MAX), 5000))]).astype(np.float32)
    got = tc.oracle_x_green(stars_lib, T)
    want = np.array([0.0 if t == 0 else np.float32(1.438776877e7 / (546.1 * float(t))) for t in T], dtype=np.float32)
    assert got.tobytes() == want.tobytes() and got.tobytes() == tc.x_green32(T).tobytes()
    assert got[0] == 0.0 and float(got[1]) * float(tc.NU_B) <= 66.1       # 500 K keeps x_B inside what e^x can take


@pytest.mark.parametrize("flags", tc.FLAGS)
def test_the_c_operator_stays_inside_the_derived_bound(stars_lib, flags):
    D, c, T = tc.operator_inputs(200000, np.random.default_rng(5 + flags))
    xg = tc.oracle_x_green(stars_lib, T)
    got = tc.oracle_colour(stars_lib, D, c, flags, xg).astype(np.float64)
    want = stars.thermal_colour(flags, D, c, T)
    one = D == np.float32(1.0)
    assert np.array_equal(got[one], c[one].astype(np.float64)), "D == 1 returns the colour bit for bit"
    assert not np.any(got[(c == 0.0)]), "a zero channel stays zero"
    if not flags & 1:           # S_f's arm: three products at most
        assert np.all(np.abs(got - want) <= 4 * tc.U * np.abs(want))
        return
    x = stars.x_green(T)[:, None] * np.array([stars.NU_R, 1.0, stars.NU_B])[None, :]
    y = x / D.astype(np.float64)[:, None]
    bound = tc.relative_bound(x, D.astype(np.float64)[:, None])
    inside = (x - y) >= -85.0
    gone = (x - y) < -87.0
    assert inside.sum() > 0.5 * inside.size and gone.sum() > 1000
    assert not np.any(got[gone]), "below e^-86 the operator returns 0"
    between = ~inside & ~gone
    assert np.all((got[between] == 0.0) | (np.abs(got[between] - want[between]) <= bound[between] * np.abs(want[between])))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    ratio = np.abs(got - want)[inside] / np.maximum(bound[inside] * np.abs(want[inside]), 1e-300)
    print(f"flags {flags}: {int(inside.sum())} channels, largest error / bound {ratio.max():.3f}, largest bound {bound[inside].max():.3g}")
    assert ratio.max() <= 1.0
    assert bound[inside].max() < 1e-4       # the bound itself is worth something: below 1e-4 of the colour everywhere


@pytest.mark.parametrize("flags", tc.FLAGS)
def test_the_numpy_float32_restatement_equals_the_c_one_bit_for_bit(stars_lib, particles_lib, flags):
    D, c, xg = tc.probe_inputs(200000, np.random.default_rng(40 + flags))
    assert (xg == 0).sum() > 100 and (D == 1).sum() > 10
    got = tc.T32(D, c, flags, xg)
    want = tc.oracle_colour(stars_lib, D, c, flags, xg)
    assert got.tobytes() == want.tobytes()
    assert tc.oracle_colour(particles_lib, D, c, flags, xg).tobytes() == want.tobytes()       # (both builds hold one operator)


# ---- the model's identities -----------------------------------------------------------------------------------------------------------
def _close(a, b, what, tol=1e-12):
    scale = np.maximum(np.abs(a), np.abs(b))
    assert np.all(np.abs(a - b) <= tol * scale), f"{what}: {np.max(np.abs(a - b) / np.maximum(scale, 1e-300)):.3g}"


def test_a_blackbody_shifted_by_d_is_a_blackbody_at_d_t():
    rng = np.random.default_rng(7)
    T = np.exp(rng.uniform(math.log(tc.T_MIN), math.log(1e6), 4000))
    D = np.exp(rng.uniform(math.log(0.2), math.log(10.0), 4000))
    A = rng.uniform(0.01, 50.0, 4000)
    scale = (planck(T) / stars.blackbody_rgb(T)).max(axis=1)        # blackbody_rgb's normalisation, the same for the three channels
    got = stars.thermal_colour(3, D, A[:, None] * stars.blackbody_rgb(T), T)
    _close(got * scale[:, None], A[:, None] * planck(D * T), "flags 3 on A blackbody_rgb(T)")


def test_two_shifts_compose_and_s_f_does_not():
    rng = np.random.default_rng(8)
    T = np.exp(rng.uniform(math.log(1000.0), math.log(1e5), 4000))
    D1, D2 = np.exp(rng.uniform(math.log(0.5), math.log(2.0), (2, 4000)))
    c = rng.uniform(0.0, 1.0, (4000, 3))
    for flags in (1, 3):
        _close(stars.thermal_colour(flags, D1, stars.thermal_colour(flags, D2, c, T), D2 * T), stars.thermal_colour(flags, D1 * D2, c, T), f"flags {flags}")
    twice, once = S(3, D1, S(3, D2, c)), S(3, D1 * D2, c)
    assert np.any(np.abs(twice - once) > 1e-3 * np.maximum(np.abs(once), 1e-3))


def test_without_the_shift_and_without_a_temperature_it_is_s_f():
    rng = np.random.default_rng(9)
    T = np.exp(rng.uniform(math.log(tc.T_MIN), math.log(tc.T_MAX), 4000))
    D = np.exp(rng.uniform(math.log(1e-3), math.log(1e3), 4000))
    c = rng.uniform(0.0, 1.0, (4000, 3))
    _close(stars.thermal_colour(2, D, c, T), S(2, D, c), "flags 2")
    assert np.array_equal(stars.thermal_colour(0, D, c, T), c)
    for flags in tc.FLAGS:
        _close(stars.thermal_colour(flags, D, c, np.zeros(4000)), S(flags, D, c), f"x_G = 0, flags {flags}")


# ---- the test that shows the feature --------------------------------------------------------------------------------------------------
def test_stars_ahead_of_a_camera_at_gamma_5_are_blackbodies_of_d_t_where_s_f_is_black(stars_lib):
    """Stars of 3000-12000 K within 10 degrees of the apex, camera at gamma = 5, shift and beaming: S_f gives exactly zero for every one of
    them, the thermal law a non-zero colour whose blue-to-red ratio is that of D T."""
    rng = np.random.default_rng(10)
    n = 500
    beta = math.sqrt(1.0 - 1.0 / 25.0)
    theta, lon = np.radians(rng.uniform(0.0, 10.0, n)), rng.uniform(-math.pi, math.pi, n)
    mag = rng.uniform(0.0, 5.0, n)
    T = np.exp(rng.uniform(math.log(3000.0), math.log(12000.0), n))
    dec, ra = np.arcsin(np.sin(theta) * np.sin(lon)), np.arctan2(np.sin(theta) * np.cos(lon), np.cos(theta))
    cat, T32 = stars.from_arrays(ra, dec, mag, T, return_temperatures=True)
    assert T32.dtype == np.float32 and np.array_equal(stars.from_arrays(ra, dec, mag, T)["dir"], cat["dir"])
    g = 5.0
    E = np.array([[g, 0, 0, g * beta], [0, 1, 0, 0], [0, 0, 1, 0], [g * beta, 0, 0, g]], dtype=np.float32)
    W, H = 128, 72
    camera = dict(sc.CAMERAS["sphere"], width=W, height=H)
    plain = stars.project(cat, E, -1, camera, 3)
    thermal = stars.project(cat, E, -1, camera, 3, temperatures=T32)
    D = thermal["D"]
    assert D.min() > 6.0 and D.max() < 9.9
    assert not np.any(plain["rgb"]), "S_f blacks out every star of the forward patch"
    assert np.all(thermal["rgb"] > 0.0)
    hot = planck(D * T32.astype(np.float64))
    # (a catalogue's colours are float32: the two channels of the ratio carry one rounding each, 2 u (1 + u) between them)
    _close(thermal["rgb"][:, 2] / thermal["rgb"][:, 0], hot[:, 2] / hot[:, 0], "blue to red", 2.001 * tc.U)
    exact = stars.thermal_colour(3, D, stars.blackbody_rgb(T32), T32)          # ... and on the colours before that rounding, to 1e-12
    _close(exact[:, 2] / exact[:, 0], hot[:, 2] / hot[:, 0], "blue to red, float64 colours")
    # ... and the C oracle, in float32, agrees: S_f exactly zero, T_f within the derived bound
    v = sc.view(camera, W, H, E, -1, 3)
    xg = tc.x_green32(T32)
    got = tc.oracle_stars_colours(stars_lib, v, cat, xg)
    dark = tc.oracle_stars_colours(stars_lib, v, cat, np.zeros(n, dtype=np.float32))
    assert got["visible"].all() and not np.any(dark["rgb"]) and np.all(got["rgb"] > 0.0)
    x = stars.x_green(T32)[:, None] * np.array([stars.NU_R, 1.0, stars.NU_B])[None, :]
    # (D itself is a float32 matrix product here: its error, a few u, moves the colour by (x / D + 2) times as much)
    bound = tc.relative_bound(x, D[:, None]) + (x / D[:, None] + 2.0) * 64 * tc.U + 8 * tc.U
    assert np.all(np.abs(got["rgb"] - thermal["rgb"]) <= bound * thermal["rgb"])


# ---- both passes: the C oracle against the model, and the cases' non-vacuity -----------------------------------------------------------
_FRAMES = {}


def _frame(events_lib, motion, name, size, interval):
    key = (motion, name, size, interval)
    if key not in _FRAMES:
        W, H = size
        camera = tc.CAMERAS[name]
        scene = eo.load_scene(tc.SCENE, motion, interval)
        _FRAMES[key] = (scene, camera, pc.scene_objects(scene, camera), sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1))
    return _FRAMES[key]


def _blank(W, H):
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    pixels["rgba"] = (40, 50, 60, 1)
    return pixels


def _in_frame(place, W, H):
    return place["visible"] & (place["X"] > -1.0) & (place["X"] < W) & (place["Y"] > -1.0) & (place["Y"] < H)


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(tc.CAMERAS))
@pytest.mark.parametrize("motion", tc.MOTIONS)
def test_the_star_cases_show_something(stars_lib, events_lib, motion, name, size):
    W, H = size
    scene, camera, _, records = _frame(events_lib, motion, name, size, -1)
    E = scene.camera_lorentz()[1]
    cat, T, groups = tc.star_case(camera, W, H, E, -1, tc.miss_pixel(records, W, H))
    xg = tc.x_green32(T)
    assert T.min() == 0.0 and (T == tc.T_MIN).any() and (T == tc.T_MAX).any()
    plain_lib = stars_lib
    for flags in tc.FLAGS:
        v = sc.view(camera, W, H, E, -1, flags)
        place = sc.oracle_place(plain_lib, v, cat)                  # S_f's colours and the positions
        thermal = tc.oracle_stars_colours(stars_lib, v, cat, xg)
        inframe = _in_frame(place, W, H)
        differs = (thermal["rgb"] != place["rgb"]).any(axis=1)
        assert not differs[xg == 0].any(), "a star without a temperature keeps S_f"
        model = stars.project(cat, E, -1, dict(camera, width=W, height=H), flags, temperatures=T)
        ok = thermal["visible"] & model["visible"] & (np.asarray(cat["rgb"]).max(axis=1) < 1e20)
        tol = 2e-3 * np.abs(model["rgb"]) + 1e-30       # (loose: D is a float32 matrix product; the operator's own bound is asserted above)
        assert np.all(np.abs(thermal["rgb"] - model["rgb"])[ok & (xg != 0)] <= tol[ok & (xg != 0)])
        if motion == "rest" or not flags & 1:
            assert not differs[place["D"] == 1.0].any()
            if not flags & 1:
                assert not differs.any(), "without the shift the colour rule is S_f"
        else:
            assert (inframe & differs).sum() >= 50 and (inframe & (xg == 0)).sum() >= 50, ((inframe & differs).sum(), (inframe & (xg == 0)).sum())
            assert not np.any(place["rgb"][groups["out of band"]]) and np.all(thermal["rgb"][groups["out of band"]] > 0.0)
            after_plain, _ = sc.oracle_pass(plain_lib, v, cat, _blank(W, H), records)
            after, counts = tc.oracle_stars_pass(stars_lib, v, cat, xg, _blank(W, H), records)
            assert after.tobytes() != after_plain.tobytes() and counts[1] > 0
        # an all-zero array is the plain pass
        after_zero, counts_zero = tc.oracle_stars_pass(stars_lib, v, cat, np.zeros(len(cat), dtype=np.float32), _blank(W, H), records)
        after_plain, counts_plain = sc.oracle_pass(plain_lib, v, cat, _blank(W, H), records)
        assert after_zero.tobytes() == after_plain.tobytes() and counts_zero == counts_plain


@pytest.mark.parametrize("size", tc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(tc.CAMERAS))
@pytest.mark.parametrize("motion", tc.MOTIONS)
def test_the_particle_cases_show_something(particles_lib, events_lib, motion, name, size):
    W, H = size
    scene, camera, objects, records = _frame(events_lib, motion, name, size, -1)
    ps, T, groups, bias = tc.particle_case(records, objects, camera, W, H, -1)
    xg = tc.x_green32(T)
    assert T.min() == 0.0 and (T == tc.T_MIN).any() and (T == tc.T_MAX).any()
    for flags in tc.FLAGS:
        for inverse_square in (False, True):
            v = pc.view(camera, W, H, -1, flags, scene.params["white_point"], inverse_square=inverse_square, depth_bias=bias)
            place = pc.oracle_place(particles_lib, v, objects, ps)
            thermal = tc.oracle_particles_colours(particles_lib, v, objects, ps, xg)
            assert np.array_equal(thermal["visible"], place["visible"])
            inframe = _in_frame(place, W, H)
            differs = (thermal["rgb"] != place["rgb"]).any(axis=1) & place["visible"]
            assert not differs[xg == 0].any()
            model = particles.project(ps, objects, camera, W, H, -1, flags, dict(inverse_square=inverse_square), temperatures=T)
            ok = thermal["visible"] & model["visible"] & (np.asarray(ps["rgb"]).max(axis=1) < 1e20) & (xg != 0)
            assert np.all(np.abs(thermal["rgb"] - model["rgb"])[ok] <= 2e-3 * np.abs(model["rgb"])[ok] + 1e-30)
            if not flags & 1:
                assert not differs.any()
            elif motion != "rest":
                assert (inframe & differs).sum() >= 50 and (inframe & (xg == 0)).sum() >= 50, ((inframe & differs).sum(), (inframe & (xg == 0)).sum())
                after_plain, _ = pc.oracle_pass(particles_lib, v, objects, ps, _blank(W, H), records)
                after, counts = tc.oracle_particles_pass(particles_lib, v, objects, ps, xg, _blank(W, H), records)
                assert after.tobytes() != after_plain.tobytes() and counts[1] > 0
            after_zero, counts_zero = tc.oracle_particles_pass(particles_lib, v, objects, ps, np.zeros(len(ps), dtype=np.float32), _blank(W, H), records)
            after_plain, counts_plain = pc.oracle_pass(particles_lib, v, objects, ps, _blank(W, H), records)
            assert after_zero.tobytes() == after_plain.tobytes() and counts_zero == counts_plain
