"""The sky of rpt_set_environment against the float64 model of tests/sky_truth.py, without a GPU (DESIGN.md "Environment map", "What
pins it besides the restatement"): (a) the C restatement tests/native/environment_oracle.c — and tests/native/window_oracle.c where a case
has windows — on every case of tests/sky_cases.py inside the float32 bound, and its lookup at crafted directions; (b) the model against
textbook formulas written with angles and speeds; (c) the wrong models the comparison must catch; (d) the caps that keep the bound and
the filters from hiding the frame.  tests/test_gpu_sky_ground_truth.py holds the device to the same bound, constants and caps, imported
from here and from sky_truth and not measured again.

Measured here, on the CPU restatement (run with -s to see every figure): the restatement's atan2f is within 2.28e-07 and its asinf
within 6.24e-08 of float64 over 18 010 directions; sky_truth asserts 4 x those (ATAN2_ERROR, ASIN_ERROR).  Every other term of the bound
is derived (sky_truth's docstring).  With them the largest error of the restatement over every case and setting is 0.14 of its bound (the
float64 model and the float32 program agree to about 1e-6 of a mapped channel), the largest share of compared pixels whose bound exceeds
2 / 255 is 0.08 % (cap 1 %), the largest undecided share 1.62 % (cap 2 %), and the smallest number of compared pixels 1313."""
import ctypes as C
import math

import numpy as np
import pytest

import doppler_model as dm
import oracle_ffi
import primitive_truth as pt
import raymap_cases as rc
import sky_cases as sc
import sky_truth as st
import window_oracle as wo


@pytest.fixture(scope="module")
def elib(tmp_path_factory):
    lib = rc.environment_oracle(tmp_path_factory.mktemp("sky_truth_e"))
    lib.rpt_environment_oracle_lookup.restype = C.c_int
    lib.rpt_environment_oracle_lookup.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def wlib(tmp_path_factory):
    return wo.build_library(tmp_path_factory.mktemp("sky_truth_w"))


# ---- the restatement's frames and the model's verdicts: computed once per case and shared -------------------------------------------------
def restatement_frame(elib, wlib, case, scene, flags, windows=None):
    """(rgba (N, 4), rgb (N, 3), hit (N,) bool or None) of the C restatement for a case's rays: it is fed what the device's kernels see —
    the objects and E re-based by the library's own rpt_orient_objects / rpt_orient_matrix where the head is turned."""
    from relativitypathtracer_amd.renderer import orient_matrix, orient_objects
    dirs, _, ypr, _ = sc.form_rays(case.form, case.frame)
    W, H = case.frame
    E = sc.device_matrix(case, scene)
    objs = None
    if any(ypr):
        E, objs = orient_matrix(E, *ypr), orient_objects(scene, *ypr)
    img = sc.image(case.image)
    if windows is not None:
        px, rgb, _, _ = wo.render(wlib, scene, W, H, windows, dirs=dirs, flags=flags, objects=objs, sky=img, sky_frame=E)
        return px["rgba"].reshape(-1, 4), rgb.reshape(-1, 3), None
    a, keep = rc.oracle_args(scene, W, H, objs)
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    hit = np.zeros(W * H, dtype=np.uint8)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    E = np.ascontiguousarray(E, dtype=np.float32)
    assert elib.rpt_environment_oracle_render(C.byref(a), dirs.ctypes.data, E.ctypes.data, img.ctypes.data, img.shape[1], img.shape[0], int(flags),
                                              hit.ctypes.data, rc.THREADS) == 0
    del keep
    return px["rgba"].reshape(-1, 4), rgb.reshape(-1, 3), hit.astype(bool)


_VERDICTS, _FRAMES = {}, {}


def case_verdict(case, interval, wlib):
    """(scene, windows, sky, hit, undecided) of a case with light delay on or off: the model's verdict, computed once."""
    key = (case.name, interval)
    if key not in _VERDICTS:
        scene = sc.scene_of(case, interval)
        windows = None
        if case.windowed:
            dirs = sc.form_rays(case.form, case.frame)[0]
            windows = wo.choose_windows(wlib, scene, *case.frame, dirs=dirs)
            assert np.isfinite(windows).any(), f"{case.name}: no window acts"
        _VERDICTS[key] = (scene, windows) + sc.verdict(case, scene, interval, windows)
    return _VERDICTS[key]


def case_frames(case, elib, wlib):
    """[(interval, flags, scene, windows, sky, hit, undecided, rgba, rgb, restatement's hit)] over sky_cases.SETTINGS, computed once."""
    if case.name not in _FRAMES:
        out = []
        for interval, flags in sc.settings(case):
            scene, windows, sky, hit, undecided = case_verdict(case, interval, wlib)
            out.append((interval, flags, scene, windows, sky, hit, undecided) + restatement_frame(elib, wlib, case, scene, flags, windows))
        _FRAMES[case.name] = out
    return _FRAMES[case.name]


def check_sky(label, case, model, sky, undecided, rgb, rgba, caps=True):
    """The assertions on one frame of a float program (restatement or device): every compared sky pixel's mapped colour within the
    model's bound and its bytes within the packs of the bound's ends; then the caps.  Returns sky_truth.compare's figures."""
    r = st.compare(model, rgb, rgba, sky)
    mask = sc.form_rays(case.form, case.frame)[1]
    rays = len(sky) if mask is None else int(mask.sum())
    share = float(undecided.sum()) / rays
    print(f"{label}: {r['n']} sky pixels compared, largest error / bound {r['ratio']:.3f}, bound above 2/255 on {r['loose']:.3%}, undecided {share:.3%}")
    i = r["worst"]
    assert r["bad"].size == 0, (label, f"{r['bad'].size} sky pixels beyond the bound; pixel {i}: got {np.asarray(rgb).reshape(-1, 3)[i]}, model {model['mapped'][i]}, "
                                       f"bound {model['tol_mapped'][i]}, u {model['u'][i]:.6f} v {model['v'][i]:.6f} D {model['D'][i]:.6f}")
    assert r["byte_bad"].size == 0, (label, "packed bytes outside the packs of the bound's ends", r["byte_bad"][:8])
    if caps:
        assert r["loose"] <= sc.CAP_LOOSE, (label, "too many compared pixels with a bound above 2 / 255", r["loose"])
        assert share <= sc.CAP_UNDECIDED, (label, "too many pixels left undecided by primitive_truth", share)
        assert r["n"] >= sc.MIN_PIXELS, (label, "too few sky pixels compared", r["n"])
        if case.form == "pano_full":
            assert sc.seam_and_poles(case, model, sky), (label, "the compared pixels miss a side of the seam or a pole row")
    return r


# ---- (a) the restatement against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.case_ids())
def test_restatement_agrees_with_the_model(elib, wlib, name):
    case = sc.CASES[name]
    for interval, flags, scene, windows, sky, hit, undecided, rgba, rgb, ohit in case_frames(case, elib, wlib):
        model = sc.model(case, interval, flags, scene.params["white_point"])
        check_sky(f"{name} interval {interval} flags {flags}", case, model, sky, undecided, rgb, rgba)
        if ohit is not None:
            assert not ohit[sky].any() and ohit[hit].all(), (name, "the restatement's hit or miss differs from the model's clear verdict")
        if case.scene == "cubes":
            assert hit.sum() > 0, (name, "no object in view")


@pytest.mark.parametrize("size", sc.IMAGES)
def test_restatement_lookup_at_crafted_directions(elib, size):
    """rpt_environment_oracle_lookup at the axes, both sides of the seam, within 1e-3 of each pole, texel centres and corners."""
    W, H = size
    img = sc.image(size)
    d = sc.crafted_directions(W, H)
    out = np.zeros((len(d), 5), dtype=np.float32)
    assert elib.rpt_environment_oracle_lookup(d.ctypes.data, len(d), img.ctypes.data, W, H, out.ctypes.data) == 0
    r = check_lookup(f"lookup {W} x {H}", d, img, out)
    assert r["held"] >= 0.95 * len(d)
    # the stated facts, exactly: u = 1/2 is +x, u = 3/4 is +z, u = 1/4 is -z, u = 0 = 1 is -x, v = 1 is +y
    m = st.lookup(d[:6], img)
    assert np.allclose(m["u"], [0.5, 1.0, 0.5, 0.5, 0.75, 0.25], atol=1e-15) and np.allclose(m["v"], [0.5, 0.5, 1.0, 0.0, 0.5, 0.5], atol=1e-15)


def check_lookup(label, d, img, out):
    """{u, v, r, g, b} of a float lookup (the restatement's, or rpt_probe which = 7) against the model's at directions d."""
    m = st.lookup(d, img)
    eu = np.abs(out[:, 0].astype(np.float64) - m["u"])
    eu = np.minimum(eu, np.abs(1.0 - eu))                                 # u = 0 and u = 1 are one meridian
    ev = np.abs(out[:, 1].astype(np.float64) - m["v"])
    ec = np.abs(out[:, 2:].astype(np.float64) - m["linear"])
    fin = np.isfinite(m["tol_linear"]).all(axis=1)
    ru, rv = float((eu / m["tol_u"]).max()), float((ev / m["tol_v"]).max())
    rc_ = float((ec[fin] / m["tol_linear"][fin]).max())
    print(f"{label}: {len(d)} directions, {int(fin.sum())} with a finite colour bound; error / bound: u {ru:.3f}, v {rv:.3f}, colour {rc_:.3f}")
    assert ru <= 1.0 and rv <= 1.0 and rc_ <= 1.0, (label, ru, rv, rc_)
    return {"held": int(fin.sum())}


def test_measured_constants():
    """The two measured constants of the bound: the restatement's atan2f and asinf against float64 (sky_truth asserts 4 x these)."""
    lib = oracle_ffi.lib()
    rng = np.random.default_rng(5)
    ds = [sc.crafted_directions(*size) for size in sc.IMAGES]
    for case in sc.CASES.values():
        d = sc.model(case, -1, 0, (1.0, 1.0, 1.0))["d"]
        ds.append(d[rng.choice(len(d), 400)])
    d = np.concatenate(ds).astype(np.float32).astype(np.float64)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    out = (C.c_float * 2)()
    worst_asin = worst_atan2 = 0.0
    for x, y, z in d:
        lib.rpt_oracle_asin_atan2(C.c_float(min(max(y, -1.0), 1.0)), C.c_float(z), C.c_float(x), out)
        worst_asin = max(worst_asin, abs(out[0] - math.asin(min(max(float(y), -1.0), 1.0))))
        worst_atan2 = max(worst_atan2, abs(out[1] - math.atan2(float(z), float(x))))
    print(f"{len(d)} directions: |atan2f - atan2| <= {worst_atan2:.3e}, |asinf - asin| <= {worst_asin:.3e}")
    assert worst_atan2 <= st.MEASURED_ATAN2_ERROR and worst_asin <= st.MEASURED_ASIN_ERROR
    assert st.ATAN2_ERROR == 4 * st.MEASURED_ATAN2_ERROR and st.ASIN_ERROR == 4 * st.MEASURED_ASIN_ERROR


def test_case_list_covers_every_axis():
    cases = list(sc.CASES.values())
    for scene in ("allsky", "cubes"):
        sub = [c for c in cases if c.scene == scene]
        assert {c.form for c in sub} == set(sc.FORMS) and {c.camera for c in sub} == set(sc.CAMERAS) and {c.sky for c in sub} == set(sc.SKIES)
        assert {c.image for c in sub} == set(sc.IMAGES)
    allsky = [c for c in cases if c.scene == "allsky"]
    assert {(c.form, c.camera) for c in allsky} == {(f, c) for f in sc.FORMS for c in sc.CAMERAS}
    assert {c.frame for c in allsky} == set(sc.FRAMES)
    assert {(c.frame, c.image) for c in allsky if c.form == "pano_full"} >= {(sc.FRAMES[0], sc.IMAGES[0]), (sc.FRAMES[1], sc.IMAGES[1])}
    assert sum(c.windowed for c in cases) >= 3
    assert {s for s in sc.SETTINGS} >= {(-1, f) for f in range(4)} | {(0, 0)}
    for size in sc.IMAGES:                                     # no mirror symmetry, in azimuth or in latitude
        img = sc.image(size).astype(int)
        assert np.abs(img - img[:, ::-1]).mean() > 10 and np.abs(img - img[::-1]).mean() > 10 and np.abs(img - np.roll(img[:, ::-1], 1, axis=1)).mean() > 10


# ---- (b) the model against textbook formulas: angles and speeds, no matrices ---------------------------------------------------------------
def _polar(axis, theta, phi):
    """The unit vector at polar angle theta from the unit vector `axis`, azimuth phi about it."""
    axis = np.asarray(axis, dtype=np.float64)
    p = np.cross(axis, [1.0, 0.0, 0.0] if abs(axis[0]) < 0.9 else [0.0, 1.0, 0.0])
    p /= np.linalg.norm(p)
    q = np.cross(axis, p)
    return math.cos(theta) * axis + math.sin(theta) * (math.cos(phi) * p + math.sin(phi) * q)


GREY = np.full((4, 8, 3), 60, dtype=np.uint8)
AXES = {"+z": np.array([0.0, 0.0, 1.0]), "oblique": sc.OBLIQUE}


@pytest.mark.parametrize("axis", list(AXES))
@pytest.mark.parametrize("beta", [0.2, 0.5, 0.95])
def test_model_aberration_and_doppler_factor(axis, beta):
    """Camera at beta along a; a pixel looking at polar angle theta from a sees the sky's direction at theta', cos theta' = (cos theta -
    beta) / (1 - beta cos theta), the azimuth about a unchanged; and D = 1 / (gamma (1 - beta cos theta)): sqrt((1 + beta) / (1 - beta))
    ahead, its inverse behind, 1 / gamma at right angles."""
    a = AXES[axis]
    v = (np.float32(beta) * a.astype(np.float32)).astype(np.float64)
    b = float(np.linalg.norm(v))
    a = v / b
    gamma = 1.0 / math.sqrt(1.0 - b * b)
    thetas = np.linspace(0.0, math.pi, 37)
    dirs = np.array([_polar(a, t, 0.8) for t in thetas])
    m = st.frame(dirs, GREY, v_cam=v, interval=-1, flags=3)
    cos_sky = m["d"] @ a
    assert np.allclose(cos_sky, (np.cos(thetas) - b) / (1.0 - b * np.cos(thetas)), atol=1e-12)
    side = m["d"] - cos_sky[:, None] * a
    want_side = dirs - np.cos(thetas)[:, None] * a
    inner = slice(1, -1)
    assert np.allclose(side[inner] / np.linalg.norm(side[inner], axis=1, keepdims=True), want_side[inner] / np.linalg.norm(want_side[inner], axis=1, keepdims=True), atol=1e-9)
    assert np.allclose(m["D"], 1.0 / (gamma * (1.0 - b * np.cos(thetas))), rtol=1e-12)
    assert m["D"][0] == pytest.approx(math.sqrt((1 + b) / (1 - b)), rel=1e-12) and m["D"][-1] == pytest.approx(math.sqrt((1 - b) / (1 + b)), rel=1e-12)
    assert m["D"][18] == pytest.approx(1.0 / gamma, rel=1e-12)
    # the colour is S_f of that factor and the tonemap of that: beaming of a grey sky by D^4 alone
    m2 = st.frame(dirs, GREY, v_cam=v, interval=-1, flags=dm.BEAMING)
    assert np.allclose(m2["colour"], (60.0 / 255.0) * m["D"][:, None] ** 4, rtol=1e-12)
    assert np.allclose(m2["mapped"], pt.tonemap(m2["colour"], (1.0, 1.0, 1.0)))


def test_model_doppler_factor_is_one_without_light_delay():
    dirs = np.array([_polar(sc.OBLIQUE, t, 0.3) for t in np.linspace(0.1, 3.0, 9)])
    for flags in range(4):
        m = st.frame(dirs, sc.image(sc.IMAGES[0]), v_cam=sc.CAMERAS["0.95c-oblique"], interval=0, flags=flags)
        assert (m["D"] == 1.0).all() and np.array_equal(m["colour"], m["linear"])
    m = st.frame(dirs, sc.image(sc.IMAGES[0]), v_cam=sc.CAMERAS["0.95c-oblique"], interval=-1, flags=0)
    assert (m["D"] == 1.0).all() and np.array_equal(m["colour"], m["linear"])


def test_model_sky_moving_with_the_camera_is_a_plain_lookup():
    rng = np.random.default_rng(3)
    dirs = rng.normal(size=(500, 3))
    img = sc.image(sc.IMAGES[1])
    v = sc.CAMERAS["0.95c-oblique"]
    m = st.frame(dirs, img, v_cam=v, v_sky=v, interval=-1, flags=3)
    n = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    assert np.allclose(m["d"], n, atol=1e-12) and np.allclose(m["D"], 1.0, rtol=1e-12)
    plain = st.lookup(dirs, img)
    assert np.allclose(m["u"], plain["u"], atol=1e-12) and np.allclose(m["colour"], plain["linear"], atol=1e-10)


def test_model_relative_velocity_of_sky_and_camera():
    """Collinear velocities add relativistically: camera at 0.5 along +z, sky at -0.4: beta_rel = 0.9 / 1.2 = 0.75."""
    b = (np.float64(np.float32(0.5)) + np.float64(np.float32(0.4))) / (1.0 + np.float64(np.float32(0.5)) * np.float64(np.float32(0.4)))
    m = st.frame(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]]), GREY, v_cam=(0.0, 0.0, 0.5), v_sky=(0.0, 0.0, -0.4), interval=-1, flags=1)
    assert m["D"][0] == pytest.approx(math.sqrt((1 + b) / (1 - b)), rel=1e-12) and m["D"][1] == pytest.approx(math.sqrt((1 - b) / (1 + b)), rel=1e-12)
    assert m["d"][2] @ np.array([0.0, 0.0, 1.0]) == pytest.approx(-b, abs=1e-12)
    assert m["a"] == pytest.approx(math.sqrt((1 + b) / (1 - b)), rel=1e-12)          # gamma (1 + beta) of the sky against the camera


def test_model_head_and_image_conventions():
    """Yaw +90 degrees looks towards +x, pitch +90 degrees towards +y, roll +90 degrees draws what was up on the left (R ey = ex); the
    image's centre column is +x, u = 3/4 is +z, row 0 is +y; a texel is returned unfiltered at u = x / W, v = 1 - y / H."""
    ez, ey = np.array([[0.0, 0.0, 1.0]]), np.array([[0.0, 1.0, 0.0]])
    h = math.pi / 2
    assert np.allclose(st.frame(ez, GREY, ypr=(h, 0, 0))["d"], [[1, 0, 0]], atol=1e-7)
    assert np.allclose(st.frame(ez, GREY, ypr=(0, h, 0))["d"], [[0, 1, 0]], atol=1e-7)
    assert np.allclose(st.frame(ey, GREY, ypr=(0, 0, h))["d"], [[1, 0, 0]], atol=1e-7)
    from relativitypathtracer_amd.renderer import rotation_matrix
    assert np.allclose(st.rotation(*sc.YPR), rotation_matrix(*sc.YPR), atol=1e-12)        # (compared, not used: the model forms its own)
    W, H = sc.IMAGES[1]
    img = sc.image(sc.IMAGES[1])
    y, x = np.mgrid[0:H, 0:W]
    u, v = x.reshape(-1) / W, 1.0 - y.reshape(-1) / H
    assert np.allclose(st.sample(img, u, v)[0], img.reshape(-1, 3) / 255.0, atol=1e-13)
    assert np.allclose(st.sample(img, np.array([1.0]), np.array([0.5]))[0], st.sample(img, np.array([0.0]), np.array([0.5]))[0])      # the seam
    m = st.lookup(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]]), img)
    assert np.allclose(m["u"], [0.75, 0.25])
    assert (st.pack([0.0, 0.5, 0.99999, 1.0, 254.9 / 255]) == [0, 127, 254, 255, 254]).all()


# ---- (c) power: wrong models the assertion of (a) must reject ---------------------------------------------------------------------------------
MUTANTS = {
    "azimuth mirrored": ("uv_of", lambda d: (0.5 + np.arctan2(-d[:, 2], d[:, 0]) / (2 * np.pi), np.arcsin(np.clip(d[:, 1], -1.0, 1.0)) / np.pi + 0.5)),
    "v flipped": ("uv_of", lambda d: (0.5 + np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi), 0.5 - np.arcsin(np.clip(d[:, 1], -1.0, 1.0)) / np.pi)),
    "boost the wrong way round": ("sky_frame", lambda vc, vs=(0.0, 0.0, 0.0): pt.boost(-np.asarray(vs, dtype=np.float64)) @ pt.boost(np.asarray(vc, dtype=np.float64))),
    "D inverted": ("doppler_factor", lambda interval, k_t: k_t / float(interval)),
    "beaming exponent off by one": ("shift_and_beam", lambda D, c, flags: dm.S64(D, c, flags) * (D[:, None] if flags & dm.BEAMING else 1.0)),
    "a half-texel offset": ("texel_coords", lambda u, v, W, H: (W * u - 0.5, H * (1.0 - v) - 0.5)),
    "no wrap at the seam": ("wrap_column", lambda x, W: np.clip(x, 0, W - 1)),
    "wrap instead of clamp in the rows": ("clamp_row", lambda y, H: y % H),
    "orientation applied transposed": ("head", lambda n, R: n @ R),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_a_wrong_model_fails_the_comparison(elib, wlib, monkeypatch, mutant):
    """Each wrong model, put in the model's place, must fail check_sky on the restatement's frame of at least one case."""
    attr, wrong = MUTANTS[mutant]
    order = sorted(sc.CASES.values(), key=lambda c: (c.scene != "allsky", c.form not in ("pano_full", "turned"), c.camera == "rest"))
    failed = None
    for case in order:
        for interval, flags, scene, windows, sky, hit, undecided, rgba, rgb, _ in case_frames(case, elib, wlib):
            with monkeypatch.context() as mp:
                mp.setattr(st, attr, wrong)
                model = sc.model(case, interval, flags, scene.params["white_point"])
                r = st.compare(model, rgb, rgba, sky)
            if r["bad"].size:
                failed = (case.name, interval, flags, int(r["bad"].size), r["n"], r["ratio"])
                break
        if failed:
            break
    assert failed is not None, f"{mutant}: no case fails"
    print(f"{mutant}: fails on {failed[0]} interval {failed[1]} flags {failed[2]}: {failed[3]} of {failed[4]} sky pixels beyond the bound, largest error / bound {failed[5]:.3g}")
    # and the right model passes that very frame
    case = sc.CASES[failed[0]]
    for interval, flags, scene, windows, sky, hit, undecided, rgba, rgb, _ in case_frames(case, elib, wlib):
        if (interval, flags) == failed[1:3]:
            assert st.compare(sc.model(case, interval, flags, scene.params["white_point"]), rgb, rgba, sky)["bad"].size == 0
