"""The star-field pass without a device: tests/native/stars_oracle.c — the C restatement of the rules, the reference of
tests/test_gpu_stars.py — against relativitypathtracer_amd.stars.project, the float64 model; the model against special relativity; the
registration of stars with the sky lookup; the round trip pixel -> direction -> pixel; and the non-vacuity of tests/stars_cases.py.

The position bound (DESIGN.md §19 "How far float32 may put a star from the float64 model") with eps = 2^-24, a = gamma (1 + beta) the
norm of the boost, is per star:
    dn  = ((2.83 a^3 + 15.9 a) a + 4) eps                the angle between the two camera directions
    pinhole:   |dX| <= 1.01 W / (2 s aspect) (1 / n.z + |n.x| / n.z^2) dn + 5 eps (|X| + W), Y likewise with H / (2 s) and n.y
    equirect:  |dX| <= (W / h_fov) (min(1.01 dn / h, 2 pi) + 100 eps) + 4 eps (|X| + W), h = hypot(n.x, n.z), X compared modulo a turn;
               |dY| <= (H / v_fov) (min(1.01 dn / h, 1.01 sqrt(2 dn)) + 20 eps) + 4 eps (|Y| + H)"""
import ctypes as C
import math

import numpy as np
import pytest

import events_oracle as eo
import stars_cases as sc
from relativitypathtracer_amd import stars
from relativitypathtracer_amd.renderer import orient_matrix

EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("stars"))


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("stars_events"))


def boost_z(beta):
    """E, camera frame -> sky frame, for a camera that moves at beta along +z through the sky's frame (float64)."""
    g = 1.0 / math.sqrt(1.0 - beta * beta)
    return np.array([[g, 0, 0, g * beta], [0, 1, 0, 0], [0, 0, 1, 0], [g * beta, 0, 0, g]], dtype=np.float64)


def direction_bound(beta):
    a = math.sqrt((1.0 + beta) / (1.0 - beta))
    return ((2.83 * a ** 3 + 15.9 * a) * a + 4.0) * EPS, a


@pytest.mark.parametrize("interval", sc.INTERVALS)
@pytest.mark.parametrize("beta", [0.0, 0.9])
@pytest.mark.parametrize("turned", [False, True])
@pytest.mark.parametrize("name", ["pinhole", "lens", "sphere", "partial"])
def test_the_c_oracle_puts_every_star_where_the_float64_model_does(lib, name, turned, beta, interval):
    W, H = 128, 72
    camera = dict(sc.CAMERAS[name], width=W, height=H, orientation=sc.YPR if turned else None)
    E = boost_z(beta).astype(np.float32)
    cat = stars.random_catalogue(2000, sc.SEED)
    got = sc.oracle_place(lib, sc.view(camera, W, H, E, interval, 0), cat)
    want = stars.project(cat, E, interval, camera)
    dn, _ = direction_bound(beta)
    n = want["n"]
    both = got["visible"] & want["visible"]
    if camera["mode"] == "pinhole":
        s = float(eo.lens_scale(camera["v_fov"])) if camera.get("v_fov") else 1.0
        both &= n[:, 2] >= 0.05
        # visibility itself agrees away from the horizon of the image plane
        assert np.array_equal(got["visible"][np.abs(n[:, 2]) > 1e-3], want["visible"][np.abs(n[:, 2]) > 1e-3])
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
            tol_y = H / v_fov * (np.minimum(1.01 * dn / h, 1.01 * math.sqrt(2 * dn)) + 20 * EPS) + 4 * EPS * (np.abs(want["Y"]) + H)
        turn = W * 2 * math.pi / h_fov
        dx = (got["X"] - want["X"] + turn / 2) % turn - turn / 2
    dy = got["Y"] - want["Y"]
    assert both.sum() > (300 if camera["mode"] == "pinhole" else 1999), both.sum()
    worst_x, worst_y = np.max(np.abs(dx[both]) / tol_x[both]), np.max(np.abs(dy[both]) / tol_y[both])
    print(f"{name} turned={turned} beta={beta} interval={interval}: {both.sum()} stars, largest |dX| / bound {worst_x:.3f}, |dY| / bound {worst_y:.3f}, "
          f"largest |dX| {np.max(np.abs(dx[both])):.3g} px")
    assert worst_x <= 1.0 and worst_y <= 1.0
    assert np.max(tol_x[both & (np.abs(want["X"] - W / 2) < W / 2)]) < 0.5      # the bound itself is below half a pixel inside the frame


@pytest.mark.parametrize("beta", [0.3, 0.9, 0.99])
def test_the_model_is_special_relativity(beta):
    """For a boost along the view axis: cos theta' = (cos theta + beta) / (1 + beta cos theta) and D = gamma (1 + beta cos theta)."""
    cat = stars.random_catalogue(2000, 3)
    p = stars.project(cat, boost_z(beta), -1, dict(mode="equirect", width=64, height=32))
    s = cat["dir"].astype(np.float64)
    cos_t = s[:, 2] / np.linalg.norm(s, axis=1)
    g = 1.0 / math.sqrt(1.0 - beta * beta)
    assert np.max(np.abs(p["n"][:, 2] - (cos_t + beta) / (1.0 + beta * cos_t))) <= 1e-12
    assert np.max(np.abs(p["D"] / (g * (1.0 + beta * cos_t)) - 1.0)) <= 1e-12
    # the transverse direction keeps its azimuth about the axis
    assert np.max(np.abs(np.arctan2(p["n"][:, 1], p["n"][:, 0]) - np.arctan2(s[:, 1], s[:, 0]))) <= 1e-9


def test_a_point_source_brightens_by_d_with_the_shift_and_by_d_squared_without():
    beta = 0.1
    cat = np.zeros(500, dtype=stars.STAR_DTYPE)
    rng = np.random.default_rng(5)
    cat["dir"] = rng.normal(size=(500, 3))
    cat["rgb"] = 0.7                                   # grey: the spectrum is flat between the red and the blue primary
    E = boost_z(beta)
    camera = dict(mode="equirect", width=64, height=32)
    plain = stars.project(cat, E, -1, camera, doppler=0)
    D = plain["D"]
    assert D.min() < 0.95 and D.max() > 1.05 and 1.0 / D.max() > stars.NU_R and 1.0 / D.min() < stars.NU_B      # green stays between the two primaries
    assert np.array_equal(plain["rgb"], cat["rgb"].astype(np.float64))
    both = stars.project(cat, E, -1, camera, doppler=3)
    assert np.max(np.abs(both["rgb"][:, 1] / (0.7 * D) - 1.0)) <= 1e-6     # (0.7 is a float32 in the catalogue)
    alone = stars.project(cat, E, -1, camera, doppler=2)
    assert np.max(np.abs(alone["rgb"] / (cat["rgb"].astype(np.float64) * (D ** 2)[:, None]) - 1.0)) <= 1e-12
    shift = stars.project(cat, E, -1, camera, doppler=1)
    assert np.max(np.abs(shift["rgb"][:, 1] / 0.7 - 1.0)) <= 1e-6          # the shift alone leaves a flat spectrum's green where it was
    off = stars.project(cat, E, 0, camera, doppler=3)
    assert np.array_equal(off["rgb"], cat["rgb"].astype(np.float64)) and np.all(off["D"] == 1.0)


def test_the_forward_hemisphere_fills_as_the_camera_speeds_up():
    cat = stars.random_catalogue(4000, 9)
    counts = [int((stars.project(cat, boost_z(b), -1, dict(mode="equirect", width=64, height=32))["n"][:, 2] > 0).sum()) for b in (0.0, 0.5, 0.9, 0.99)]
    assert counts[0] < counts[1] < counts[2] < counts[3] and abs(counts[0] - 2000) < 150 and counts[3] > 3900, counts
    # with light delay off nothing is aberrated by the boost's time row: the spatial block alone
    still = stars.project(cat, boost_z(0.9), 0, dict(mode="equirect", width=64, height=32))
    assert abs(int((still["n"][:, 2] > 0).sum()) - counts[0]) == 0


@pytest.mark.parametrize("interval", sc.INTERVALS)
@pytest.mark.parametrize("beta", [0.0, 0.9])
@pytest.mark.parametrize("turned", [False, True])
def test_a_stars_direction_looks_its_own_dir_up_in_the_sky(lib, turned, beta, interval):
    """Registration: the camera direction the pass gives a star, sent through the sky lookup's own transform (environment_oracle.c's
    k = E' (interval, n), d = normalize(k.yzw)), is the star's dir again, to a^2 dn + (16 a^2 + 4) eps."""
    W, H = 128, 72
    camera = dict(mode="equirect", width=W, height=H, orientation=sc.YPR if turned else None)
    E = boost_z(beta).astype(np.float32)
    cat = stars.random_catalogue(2000, sc.SEED)
    v = sc.view(camera, W, H, E, interval, 0)
    got = sc.oracle_place(lib, v, cat)
    assert got["visible"].all()
    n = np.ascontiguousarray(got["n"], dtype=np.float32)
    back = np.zeros_like(n)
    e_turned = np.ascontiguousarray(np.array(v.E[:], dtype=np.float32))
    assert lib.rpt_stars_oracle_sky_direction(e_turned.ctypes.data, interval, n.ctypes.data, len(n), back.ctypes.data) == 0
    s = cat["dir"].astype(np.float64)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    dn, a = direction_bound(beta)
    bound = a * a * dn + (16 * a * a + 4) * EPS
    worst = float(np.max(np.linalg.norm(back.astype(np.float64) - s, axis=1)))
    print(f"turned={turned} beta={beta} interval={interval}: largest |d - dir| {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound


@pytest.mark.parametrize("turned", [False, True])
@pytest.mark.parametrize("name", ["pinhole", "lens", "sphere", "partial"])
def test_a_star_at_a_pixels_own_direction_puts_its_heaviest_tap_on_that_pixel(lib, name, turned):
    W, H = 16, 9
    camera = dict(sc.CAMERAS[name], width=W, height=H, orientation=sc.YPR if turned else None)
    E = np.eye(4, dtype=np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    n = sc.pixel_direction(camera, W, H, xs.reshape(-1), ys.reshape(-1))
    cat = np.zeros(W * H, dtype=stars.STAR_DTYPE)
    cat["dir"] = sc.sky_direction(camera, E, -1, n)         # E' (interval, n): after re-basing by the orientation
    cat["rgb"] = 1.0
    v = sc.view(camera, W, H, E, -1, 0)
    if turned:
        assert np.array_equal(np.array(v.E[:], dtype=np.float32).reshape(4, 4), orient_matrix(E, *sc.YPR))
    got = sc.oracle_place(lib, v, cat)
    assert got["visible"].all()
    assert np.array_equal(np.floor(got["X"] + 0.5).astype(int), xs.reshape(-1)) and np.array_equal(np.floor(got["Y"] + 0.5).astype(int), ys.reshape(-1))
    assert np.max(np.abs(got["X"] - xs.reshape(-1))) < 1e-3 and np.max(np.abs(got["Y"] - ys.reshape(-1))) < 1e-3
    # ... and through the splat: one star alone lights its own pixel most, every pixel a miss
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    records = np.zeros(W * H, dtype=eo.EVENT_DTYPE)
    records["object"] = -1
    for k in (0, W - 1, W * (H // 2) + W // 2, W * H - 1):
        after, counts = sc.oracle_pass(lib, v, cat[k:k + 1], pixels, records)
        assert counts[0] == 1 and counts[1] >= 1 and int(np.argmax(after["rgba"][:, 1])) == k


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(sc.CAMERAS))
@pytest.mark.parametrize("motion", sc.MOTIONS)
@pytest.mark.parametrize("scene_name", sc.SCENES)
def test_the_shared_cases_show_something(lib, events_lib, scene_name, motion, name, size):
    """What tests/test_gpu_stars.py assumes of every case, on CPU event frames: hit and miss pixels, a pass that changes pixels and
    leaves stars out, and crafted stars that do what they are there for."""
    W, H = size
    camera = sc.CAMERAS[name]
    scene = eo.load_scene(scene_name, motion, -1)
    records = sc.cpu_events(events_lib, scene, W, H, camera).reshape(-1)
    hit = records["object"] >= 0
    assert hit.any() and (~hit).any(), f"{scene_name} {motion} {name} {W}x{H}: {int(hit.sum())} hit pixels of {hit.size}"
    E = scene.camera_lorentz()[1]
    miss = np.nonzero(~hit.reshape(H, W)[2:H - 2, 2:W - 2])
    pile = (int(miss[1][0]) + 2, int(miss[0][0]) + 2)
    cat, groups = sc.catalogue(camera, W, H, E, -1, pile)
    pixels = np.zeros(W * H, dtype=[("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
    pixels["rgba"] = (40, 50, 60, 1)
    for flags in sc.FLAGS:
        v = sc.view(camera, W, H, E, -1, flags)
        after, (inside, changed) = sc.oracle_pass(lib, v, cat, pixels, records)
        # (the full sphere with its wrapping columns leaves no star out: every direction has a tap in the frame)
        assert (inside == len(cat) if name == "sphere" else 0 < inside < len(cat)) and changed > 0
        same = after["rgba"] == pixels["rgba"]
        assert same[hit].all() and same[:, 3].all() and np.array_equal(after["x"], pixels["x"]) and np.array_equal(after["unspecified"], pixels["unspecified"])
        place = sc.oracle_place(lib, v, cat)
        assert not np.any(place["rgb"][groups["zero colour"]])
        if not flags & 1:           # (a shift may move any one colour out of the band; without it:)
            assert np.all(place["rgb"][groups["1e30"]] > 65536.0)
            k = pile[1] * W + pile[0]
            assert after["rgba"][k, 0] == 255 and after["rgba"][k, 1] == 255, "1000 stars on one pixel saturate it"
        if camera["mode"] == "pinhole":
            assert not place["visible"][groups["behind"]].any()
        else:
            assert place["visible"][groups["seam"]].all() and place["visible"][groups["poles"]].all()
        if motion == "0.9c" and flags & 1:
            assert not np.any(place["rgb"][groups["out of band"]]), "a red star ahead of a camera at 0.9 c is shifted out of the band"
    # with light delay off the pass is the rest pass of the spatial block, whatever the flags
    v0, v3 = sc.view(camera, W, H, E, 0, 0), sc.view(camera, W, H, E, 0, 3)
    assert sc.oracle_pass(lib, v0, cat, pixels, records)[0].tobytes() == sc.oracle_pass(lib, v3, cat, pixels, records)[0].tobytes()
